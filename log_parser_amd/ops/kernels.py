"""Torch-facing wrappers of the native kernels.

Each op takes torch tensors; CUDA (HIP) tensors run the gfx950 kernel on the current stream,
CPU tensors run the host twin compiled from the same source (``csrc/kernels/lp_core.h``).
There is no silent fallback: a CUDA tensor with a missing extension raises.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from ..native import N

# pad every device text buffer so vector loads past the end stay in bounds
TEXT_PAD = 64
NL_TILE = 16384


def _s(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream if t.is_cuda else 0


def _p(t: Optional[torch.Tensor]) -> int:
    return 0 if t is None else t.data_ptr()


def padded_len(nbytes: int) -> int:
    return ((max(nbytes, 1) + NL_TILE - 1) // NL_TILE) * NL_TILE + TEXT_PAD


def newline_positions(text: torch.Tensor, nbytes: int) -> torch.Tensor:
    """Positions of every '\\n' in text[0:nbytes] (int64, ascending; host twin)."""
    c = N.nl_positions_host(text.data_ptr(), nbytes, 0)
    pos = torch.empty(c, dtype=torch.int64)
    N.nl_positions_host(text.data_ptr(), nbytes, pos.data_ptr())
    return pos


class _LineIndexWs:
    """Per (device, stream) scratch of the line index: tile counts + offsets, "\\r\\n" flags and
    each tile's first line end (k_line_fix), the per-tile newline bitmasks (256 words = 2 KiB per
    16 KiB tile), then the scan scratch. Grow-only; stream order makes reuse safe."""
    SCAN_TMP = 1 << 20           # bytes of scan scratch in the workspace layout (csrc/bind.cpp passes the same)
    WORDS_PER_TILE = 4 + 256     # int64 words per tile (csrc/kernels/line_index.hip line_index_dev)
    _all: dict = {}

    @classmethod
    def get(cls, text: torch.Tensor, ntiles: int) -> Tuple[int, int]:
        key = (text.device, _s(text))
        buf = cls._all.get(key)
        w = cls.WORDS_PER_TILE
        if buf is None or buf.numel() < w * ntiles + cls.SCAN_TMP // 8:
            cap = max(ntiles * 5 // 4, 1024)
            buf = cls._all[key] = torch.empty(w * cap + cls.SCAN_TMP // 8, dtype=torch.int64, device=text.device)
        return buf.data_ptr(), (buf.numel() - cls.SCAN_TMP // 8) // w


# lines per byte seen so far (grows only): capacity of the line index outputs, so the one-pass
# kernel rarely needs a second pass; a text with more lines than that re-runs with the exact count
_LINES_PER_BYTE = [1.0 / 48]

import threading as _threading

_count_read = _threading.local()     # per thread: the pinned 24-byte count buffer + its event


def _count_read_slot(device: torch.device):
    """(pinned int64[3], event) reused by this thread's line-index count reads on ``device`` (a
    fresh pinned allocation and event per call cost host time on config 2's critical path; the
    buffer is read before the call returns, so one per thread and device suffices)."""
    slots = getattr(_count_read, "slots", None)
    if slots is None:
        slots = _count_read.slots = {}
    slot = slots.get(device.index)
    if slot is None:
        slot = slots[device.index] = (torch.empty(3, dtype=torch.int64, pin_memory=True), torch.cuda.Event())
    return slot
LINE_BLK_SHIFT = 12


def _line_index_dev(text: torch.Tensor, nbytes: int, trim: bool, before_read=None, fused=None,
                    early_first: bool = False):
    """k_nl_count, k_tile_scan, k_nl_lines, k_line_fix (+ k_line_trim): (starts, lens, n_newlines,
    last_newline, kept, blk) with ONE host read; blk = the coarse 4 KiB block -> line index.
    ``before_read()`` runs once, after the launches and before that read: work it queues (the
    literal prefilter, which needs no line index) runs on the GPU while the host waits.
    ``fused(nlp)`` instead launches the literal prefilter FIRST with the line index's first pass
    folded into its read of the text (nlp = the pass-1 outputs, zeroed): k_nl_count does not run.
    ``early_first``: before_read() queues its work on ANOTHER stream -- it then runs before the
    count copy is even set up, so that work is launched as soon as the line index is."""
    dev = text.device
    nt = N.line_index_tiles(nbytes)
    cap = int(nbytes * _LINES_PER_BYTE[0] * 1.25) + 1024
    blk = torch.empty((max(nbytes, 1) >> LINE_BLK_SHIFT) + 2, dtype=torch.int32, device=dev)
    counted = False
    while True:
        cap = min(cap, nbytes + 1)
        starts = torch.empty(cap, dtype=torch.int64, device=dev)
        lens = torch.empty(cap, dtype=torch.int32, device=dev)
        info = torch.empty(3, dtype=torch.int64, device=dev)
        wp, wcap = _LineIndexWs.get(text, nt)
        if fused is not None:
            fused(N.line_index_pass1(wp, wcap, nbytes, _s(text)))
            fused = None
            counted = True            # a re-run (more lines than the capacity) reuses pass 1's outputs
        N.line_index_dev(text.data_ptr(), nbytes, wp, wcap, starts.data_ptr(), lens.data_ptr(), cap, info.data_ptr(),
                         trim, blk.data_ptr(), blk.numel(), _s(text), counted)
        if before_read is not None:
            # the counts travel to pinned memory behind the line index only; the host then waits
            # for that copy, not for the work before_read() queued after it
            if early_first:
                before_read()
            hinfo, done = _count_read_slot(dev)
            hinfo.copy_(info, non_blocking=True)
            done.record()
            if not early_first:
                before_read()
            before_read = None
            done.synchronize()
            n_nl, last, kept = hinfo.tolist()
        else:
            n_nl, last, kept = info.tolist()
        if n_nl + 1 <= cap:
            _LINES_PER_BYTE[0] = max(_LINES_PER_BYTE[0], (n_nl + 1) / max(nbytes, 1))
            return starts, lens, n_nl, last, kept, blk
        cap = n_nl + 1


def _with_blk(ls: torch.Tensor, blk: torch.Tensor, nbytes: int) -> torch.Tensor:
    """Attach the coarse block index to the line-start tensor the caller gets (reused by
    ``line_block_index`` for the same object; any other tensor recomputes it)."""
    ls._lp_blk = (blk, nbytes)
    return ls


def split_lines(text: torch.Tensor, nbytes: int, before_read=None, fused=None,
                early_first: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """Java ``logs.split("\\\\r?\\\\n")`` line index (AnalysisService.java:53).

    Returns (line_start int64[L], line_len int32[L]); trailing empty lines removed; input
    without any newline is one line (possibly empty). GPU: one read of the text + its newline bitmask, five small
    launches, one 24-byte host read (csrc/kernels/line_index.hip).
    """
    dev = text.device
    if text.is_cuda:
        if nbytes == 0:
            return torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        starts, lens, _, _, L, blk = _line_index_dev(text, nbytes, trim=True, before_read=before_read, fused=fused,
                                                     early_first=early_first)
        return _with_blk(starts[:L], blk, nbytes), lens[:L]
    nl = newline_positions(text, nbytes)
    if nl.numel() == 0:
        return (torch.zeros(1, dtype=torch.int64, device=dev),
                torch.full((1,), nbytes, dtype=torch.int32, device=dev))
    zero = torch.zeros(1, dtype=torch.int64, device=dev)
    starts = torch.cat([zero, nl + 1])
    ends = torch.cat([nl, torch.full((1,), nbytes, dtype=torch.int64, device=dev)])
    prev = text[(nl - 1).clamp(min=0)]
    cr = (nl > starts[:-1]) & (prev == 13)
    ends[:-1] -= cr.to(torch.int64)
    lens = ends - starts
    nz = torch.nonzero(lens > 0)
    L = int(nz[-1].item()) + 1 if nz.numel() else 0
    return starts[:L].contiguous(), lens[:L].to(torch.int32).contiguous()


def split_chunk_lines(text: torch.Tensor, nbytes: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Line index of a chunk made of complete lines (streaming): no trailing-empty trimming; a
    final '\\n' terminates the last line instead of opening an empty one."""
    dev = text.device
    if text.is_cuda and nbytes > 0:
        starts, lens, n_nl, last, _, blk = _line_index_dev(text, nbytes, trim=False)
        L = n_nl + 1 - (1 if n_nl and last == nbytes - 1 else 0)
        return _with_blk(starts[:L], blk, nbytes), lens[:L]
    nl = newline_positions(text.cpu(), nbytes).to(dev)
    zero = torch.zeros(1, dtype=torch.int64, device=dev)
    starts = torch.cat([zero, nl + 1])
    ends = torch.cat([nl, torch.full((1,), nbytes, dtype=torch.int64, device=dev)])
    if nl.numel():
        prev = text[(nl - 1).clamp(min=0)]
        cr = (nl > starts[:-1]) & (prev == 13)
        ends[:-1] -= cr.to(torch.int64)
    L = starts.numel()
    if nl.numel() and int(nl[-1].item()) == nbytes - 1:
        L -= 1
    return starts[:L].contiguous(), (ends - starts)[:L].to(torch.int32).contiguous()




def line_block_index(line_start: torch.Tensor, nbytes: int) -> torch.Tensor:
    """blk[b] = line containing byte b << 12 (int32), for O(log lines-per-4KiB) line lookups
    (already built by the GPU line index for the tensors ``split_lines`` returns)."""
    cached = getattr(line_start, "_lp_blk", None)
    if cached is not None and cached[1] == nbytes:
        return cached[0]
    nblk = (max(nbytes, 1) >> LINE_BLK_SHIFT) + 2
    blk = torch.empty(nblk, dtype=torch.int32, device=line_start.device)
    N.blk_index(line_start.data_ptr(), line_start.numel(), nblk, blk.data_ptr(), _s(line_start), line_start.is_cuda)
    return blk


def prefilter(text, nbytes, pf_tuple, line_start, cap: int, grid: int = 2048) -> torch.Tensor:
    """Literal prefilter -> (regex << 32 | line) candidates (unverified, may repeat).

    GPU: k_prefilter streams the text and stages bloom gram hits (position, gram length);
    k_pf_verify then checks whole literals, one lane per hit, reading the gram-hit count on the
    device (grid-stride) -- both counts come back in ONE host read.
    """
    nlines = line_start.numel()
    if text.is_cuda:
        dev = text.device
        gcap = cap
        blk = line_block_index(line_start, nbytes)
        while True:
            gh = torch.empty(max(gcap, 1), dtype=torch.int64, device=dev)
            cand = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
            cnt = torch.zeros(2, dtype=torch.int64, device=dev)        # [gram hits, candidates]
            N.prefilter_dev(text.data_ptr(), nbytes, pf_tuple, line_start.data_ptr(), nlines, gh.data_ptr(), gcap,
                            cnt.data_ptr(), grid, _s(text))
            N.pf_verify_dev(gh.data_ptr(), gcap, text.data_ptr(), nbytes, pf_tuple, line_start.data_ptr(), nlines,
                            blk.data_ptr(), cand.data_ptr(), cap, cnt.data_ptr() + 8, _s(text), cnt.data_ptr(),
                            max(16, min(8192, nbytes >> 13)))   # grid-stride over the device count
            c = cnt.cpu()
            g, k = int(c[0]), int(c[1])
            if g <= gcap and k <= cap:
                return cand[:k]
            gcap, cap = max(gcap, g), max(cap, k)
    while True:
        cand = torch.empty(max(cap, 1), dtype=torch.int64)
        c = N.prefilter_host(text.data_ptr(), nbytes, pf_tuple, line_start.data_ptr(), nlines, cand.data_ptr(), cap)
        if c <= cap:
            return cand[:c]
        cap = c


def scan(text, line_start, line_len, regs: torch.Tensor, dfa_tuple, cap: int) -> torch.Tensor:
    nlines = line_start.numel()
    if regs.numel() == 0 or nlines == 0:
        return torch.empty(0, dtype=torch.int64, device=text.device)
    if text.is_cuda:
        while True:
            out = torch.empty(max(cap, 1), dtype=torch.int64, device=text.device)
            cnt = torch.zeros(1, dtype=torch.int64, device=text.device)
            N.scan_dev(text.data_ptr(), line_start.data_ptr(), line_len.data_ptr(), nlines, regs.data_ptr(),
                       regs.numel(), dfa_tuple, out.data_ptr(), cap, cnt.data_ptr(), _s(text))
            c = int(cnt.item())
            if c <= cap:
                return out[:c]
            cap = c
    while True:
        out = torch.empty(max(cap, 1), dtype=torch.int64)
        c = N.scan_host(text.data_ptr(), line_start.data_ptr(), line_len.data_ptr(), nlines, regs.data_ptr(),
                        regs.numel(), dfa_tuple, out.data_ptr(), cap)
        if c <= cap:
            return out[:c]
        cap = c


def scan_multi(text, nbytes: int, line_start, line_len, pass_tuple, cap: int, grid: int = 1024) -> torch.Tensor:
    """Literal-free regexes of one scan pass (<= 4 multi-regex DFA groups) over every line ->
    (regex << 32 | line) hits, already verified."""
    nlines = line_start.numel()
    if nlines == 0:
        return torch.empty(0, dtype=torch.int64, device=text.device)
    while True:
        out = torch.empty(max(cap, 1), dtype=torch.int64, device=text.device)
        if text.is_cuda:
            cnt = torch.zeros(1, dtype=torch.int64, device=text.device)
            N.scan_multi(text.data_ptr(), nbytes, line_start.data_ptr(), line_len.data_ptr(), nlines, pass_tuple,
                         out.data_ptr(), cap, cnt.data_ptr(), grid, _s(text), True)
            c = int(cnt.item())
        else:
            c = N.scan_multi(text.data_ptr(), nbytes, line_start.data_ptr(), line_len.data_ptr(), nlines, pass_tuple,
                             out.data_ptr(), cap, 0, 0, 0, False)
        if c <= cap:
            return out[:c]
        cap = c


def nfa_features(groups: torch.Tensor, lines: torch.Tensor, L: int, text, line_start, line_len,
                 group_list: torch.Tensor, ncls: int) -> torch.Tensor:
    """Context features via the MFMA NFA kernel (``group_list`` = the groups of the 4 context
    regexes, one launch each: a group ORs its members' bits into the line's byte): uint8 bits per line."""
    feat = torch.zeros(max(L, 1), dtype=torch.uint8, device=text.device)
    if lines.numel():
        for k in range(group_list.numel()):
            N.nfa(groups.data_ptr(), group_list[k:k + 1].data_ptr(), 1, ncls, lines.data_ptr(), lines.numel(),
                  text.data_ptr(), line_start.data_ptr(), line_len.data_ptr(), feat.data_ptr(), 0, 0, 0, _s(text),
                  text.is_cuda)
    return feat


def nfa_scan(groups: torch.Tensor, group_list: torch.Tensor, ncls: int, text, line_start, line_len,
             cap: int) -> torch.Tensor:
    """All lines x NFA groups -> (regex << 32 | line) hits (MFMA kernel on GPU, bitset twin on CPU)."""
    nl = line_start.numel()
    if group_list.numel() == 0 or nl == 0:
        return torch.empty(0, dtype=torch.int64, device=text.device)
    while True:
        out = torch.empty(max(cap, 1), dtype=torch.int64, device=text.device)
        if text.is_cuda:
            cnt = torch.zeros(1, dtype=torch.int64, device=text.device)
            N.nfa(groups.data_ptr(), group_list.data_ptr(), group_list.numel(), ncls, 0, nl, text.data_ptr(),
                  line_start.data_ptr(), line_len.data_ptr(), 0, out.data_ptr(), cap, cnt.data_ptr(), _s(text), True)
            c = int(cnt.item())
        else:
            c = N.nfa(groups.data_ptr(), group_list.data_ptr(), group_list.numel(), ncls, 0, nl, text.data_ptr(),
                      line_start.data_ptr(), line_len.data_ptr(), 0, out.data_ptr(), cap, 0, 0, False)
        if c <= cap:
            return out[:c]
        cap = c


# ---------------------------------------------------------------------------------------------
# post-match pipeline (csrc/kernels/lp_post.hip): hit CSR, events, frequency ranks, features

class Uploader:
    """Several small host arrays -> device with ONE async H2D copy through a grow-only pinned
    buffer (line index, segment table, frequency carry of a request batch). CPU: zero-copy views.
    Reusing the pinned buffer is safe: every batch ends with a blocking read of its results,
    which orders after this copy on the same stream."""

    def __init__(self, device: torch.device):
        self.device = device
        self.pinned: Optional[torch.Tensor] = None

    def __call__(self, arrays):
        import numpy as np
        arrays = [np.ascontiguousarray(a) for a in arrays]
        if self.device.type != "cuda":
            return [torch.from_numpy(a) for a in arrays]
        offs, o = [], 0
        for a in arrays:
            offs.append(o)
            o += (a.nbytes + 255) // 256 * 256
        o = max(o, 256)
        if self.pinned is None or self.pinned.numel() < o:
            self.pinned = torch.empty(max(o * 5 // 4, 1 << 16), dtype=torch.uint8, pin_memory=True)
        hv = self.pinned.numpy()
        for a, off in zip(arrays, offs):
            hv[off:off + a.nbytes] = a.reshape(-1).view(np.uint8)
        dev = torch.empty(o, dtype=torch.uint8, device=self.device)
        dev.copy_(self.pinned[:o], non_blocking=True)
        return [dev[off:off + a.nbytes].view(_TORCH_DTYPE[a.dtype.str]) for a, off in zip(arrays, offs)]


_TORCH_DTYPE = {"<i8": torch.int64, "<i4": torch.int32, "<u1": torch.uint8, "<f8": torch.float64, "|u1": torch.uint8,
                "|b1": torch.bool}


class Workspace:
    """Grow-only device scratch buffer for the post-match kernels' temporaries (rocPRIM temp
    storage, sort ping-pong buffers, window difference array). One per engine; stream-ordered
    reuse is safe because every batch ends with a host read of its results."""

    def __init__(self, device: torch.device):
        self.device = device
        self.buf: Optional[torch.Tensor] = None

    def get(self, nbytes: int) -> Tuple[int, int]:
        if self.buf is None or self.buf.numel() < nbytes:
            self.buf = torch.empty(max(int(nbytes * 5 // 4), 1 << 20), dtype=torch.uint8, device=self.device)
        return self.buf.data_ptr(), self.buf.numel()

    def ptr(self) -> Tuple[int, int]:
        return (0, 0) if self.buf is None else (self.buf.data_ptr(), self.buf.numel())


def _run_ws(call, ws: Optional[Workspace]):
    """Device calls report the workspace they need and run only when it suffices."""
    p, n = ws.ptr()
    need = call(p, n)
    if need > n:
        p, n = ws.get(need)
        call(p, n)


def ev_tables(tabs: dict, segs, nkeys: int, npat: int) -> tuple:
    return (tabs["prim_off"].data_ptr(), tabs["prim_pats"].data_ptr(), tabs["freq_key"].data_ptr(),
            tabs["ctx_before"].data_ptr(), tabs["ctx_after"].data_ptr(), segs.lo.data_ptr(), segs.hi.data_ptr(),
            segs.own_lo.data_ptr(), segs.own_hi.data_ptr(), segs.lo.numel(), nkeys, N.bits_for(max(npat, 1)))


def post_hits(cand: torch.Tensor, pre_from: int, L: int, R: int, text, line_start, line_len, dfa_tuple,
              evt: tuple, ws: Optional[Workspace]):
    """Candidates -> (hits, hit_line, hit_off, ev_cnt, ev_end, n_hits, n_events).

    ``cand[:pre_from]`` are prefilter candidates still to DFA-verify, ``cand[pre_from:]`` hits of
    engines that verified already (scan / MFMA NFA / host fallback). Duplicates are allowed.
    Output hits are sorted unique (regex << 32 | line); one 16-byte host read for the counts."""
    dev = cand.device
    n = cand.numel()
    m = max(n, 1)
    hits = torch.empty(m, dtype=torch.int64, device=dev)
    hit_line = torch.empty(m, dtype=torch.int32, device=dev)
    hit_off = torch.empty(R + 1, dtype=torch.int64, device=dev)
    ev_cnt = torch.empty(m, dtype=torch.int64, device=dev)
    ev_end = torch.empty(m, dtype=torch.int64, device=dev)
    counters = torch.empty(2, dtype=torch.int64, device=dev)      # written by the pipeline
    lbits, rbits = N.bits_for(max(L, 1)), N.bits_for(max(R, 1))

    def call(wp, wn):
        return N.post_hits(cand.data_ptr(), n, pre_from, lbits, rbits, R, text.data_ptr(), line_start.data_ptr(),
                           line_len.data_ptr(), dfa_tuple, evt, hits.data_ptr(), hit_line.data_ptr(),
                           hit_off.data_ptr(), ev_cnt.data_ptr(), ev_end.data_ptr(), counters.data_ptr(), wp, wn,
                           _s(cand), cand.is_cuda, 0, 0)

    if cand.is_cuda:
        _run_ws(call, ws)
        c = counters.cpu()
    else:
        call(0, 0)
        c = counters
    nh, ne = int(c[0]), int(c[1])
    return hits[:nh], hit_line, hit_off, ev_cnt, ev_end, nh, ne


class MatchArena:
    """Fixed-capacity device buffers of every matcher of one batch + their append counters
    (GPU): gram hits (k_prefilter), prefilter candidates (k_pf_verify), verified hits of the
    self-verifying engines (scan passes, single-DFA scan, MFMA NFA). Nothing is read back until
    the hit CSR is built, so matching + verify + CSR + event count cost ONE host read
    (``match_and_hits``); capacities follow the largest per-line rates seen so far, and a batch
    that overflows one re-runs with its exact counts."""

    def __init__(self):
        # starting rates per line (an underestimate costs one re-run of the matchers; an
        # overestimate costs post-match work on every batch, which covers the capacity); "ev":
        # events, only for steps that defer the count read (``match_and_hits(defer=True)``)
        self.rate = {"gram": 0.08, "cand": 0.03, "ver": 0.01, "ev": 0.01}
        self.last: dict = {}            # counts of the latest batch (diagnostics)

    def caps(self, L: int) -> dict:
        return {k: int(L * r * 1.25) + 512 for k, r in self.rate.items()}

    @staticmethod
    def overflow(counts: list, caps: dict) -> bool:
        """counts = [gram, cand, ver, nh, ne] of a deferred step vs its capacities."""
        g, k, v, _, ne = counts
        return g > caps["gram"] or k > caps["cand"] or v > caps["ver"] or ne > caps["ev"]

    def learn_deferred(self, L: int, counts: list) -> None:
        g, k, v, nh, ne = counts
        self.last = {"lines": L, "gram_hits": g, "prefilter_candidates": k, "scan_hits": v, "hits": nh, "events": ne}
        self.learn(L, {"gram": g, "cand": k, "ver": v, "ev": ne}, overflow=False)

    def learn(self, L: int, counts: dict, overflow: bool) -> None:
        """Overflow: the exact rates. Otherwise decay toward what batches need (the hit sort
        covers the whole capacity, so slack costs sort time)."""
        for k, c in counts.items():
            r = c / max(L, 1)
            self.rate[k] = max(r, self.rate[k] if overflow else self.rate[k] * 0.5, 1e-4)


def _pf_events(stream: "torch.cuda.Stream"):
    """(fork, done) events of this thread's early prefilter on ``stream`` (EarlyPrefilter): a
    consumer that waits on a later record of `done` waits on a later point of the same stream, so
    reuse never waits too little."""
    ev = getattr(_count_read, "pf_events", None)
    if ev is None:
        ev = _count_read.pf_events = {}
    e = ev.get(stream.cuda_stream)
    if e is None:
        e = ev[stream.cuda_stream] = (torch.cuda.Event(), torch.cuda.Event())
    return e


class EarlyPrefilter:
    """The literal prefilter launched before the line index is known on the host (it reads only
    the text): gram hits + the arena counters, handed to ``match_and_hits``."""

    def __init__(self, text, nbytes: int, tabs: dict, arena: "MatchArena", pf_grid: int, nlp=None,
                 stream: Optional["torch.cuda.Stream"] = None):
        L_est = int(nbytes * _LINES_PER_BYTE[0]) + 1
        self.cap = arena.caps(L_est)["gram"]
        self.gh = torch.empty(self.cap, dtype=torch.int64, device=text.device)
        self.cnt = torch.zeros(7, dtype=torch.int64, device=text.device)
        self.done = None
        st = _s(text)
        if stream is not None and nlp is None and text.is_cuda:
            # on its own stream: the rest of the line index (line starts / lengths, after the host's
            # line-count read) and the literal-free scans run beside it; match_and_hits waits for
            # `done` before the candidates' verification (config 2: the chains overlap)
            # (this thread's two events of this stream, reused)
            fork, done = _pf_events(stream)
            fork.record(torch.cuda.current_stream(text.device))
            stream.wait_event(fork)
            st = stream.cuda_stream
        N.prefilter_dev(text.data_ptr(), nbytes, tabs["pf"], 0, 0, self.gh.data_ptr(), self.cap, self.cnt.data_ptr(),
                        pf_grid, st, nlp)
        if st != _s(text):
            self.done = done
            self.done.record(stream)
            for t in (self.gh, self.cnt, text):     # (allocator bookkeeping: after the launch)
                t.record_stream(stream)


def match_and_hits(text, nbytes: int, line_start, line_len, tabs: dict, R: int, evt: tuple, arena: MatchArena,
                   ws: Optional[Workspace], pf_grid: int, scan_grid, timings=None, tick=None, side=None,
                   early: Optional[EarlyPrefilter] = None, defer: bool = False,
                   inject: Optional[torch.Tensor] = None, host_side=None):
    """GPU: every matcher appends to the arena, then the post-match hit pipeline reads the device
    counters itself -> (hits, hit_line, hit_off, ev_cnt, ev_end, nh, ne) with ONE host read.

    ``defer``: no read -> (hits, hit_line, hit_off, ev_cnt, ev_end, hit capacity, device counters
    [gram, cand, ver, nh, ne], capacities incl. "ev"); the caller checks the counters against the
    capacities later (``MatchArena.overflow``) and re-runs with ``arena.learn``.

    ``side`` = (stream, fork event, join event): the self-verifying engines (literal-free DFA scan,
    single-DFA scan, MFMA NFA) run on that stream, concurrently with the literal prefilter chain
    (block index -> prefilter -> verify) on the current one; both join before the hit pipeline.
    A small request's kernels are latency-bound and leave most CUs idle, so the two chains
    overlap almost fully.

    ``inject``: device keys verified elsewhere (the host backtracker's side path,
    ``Engine.host_hits``), appended to the verified-hit buffer like a self-verifying engine's.

    ``host_side`` = (ops.side_path.HostSide, host bytes): the backtracker regexes fed by their
    relaxed automata export their device candidates to the host and get the verified keys back,
    all queued (side_path.hip); without it their device keys are only dropped (the host side path
    ran for them before, ``inject``)."""
    dev = text.device
    L = line_start.numel()
    st = _s(text)
    lbits, rbits = N.bits_for(max(L, 1)), N.bits_for(max(R, 1))
    scans = bool(tabs["scan_passes"]) or bool(tabs["scan_regs"].numel()) or \
        any(g.numel() for g in tabs["nfa_scan_lists"].values())
    ninj = 0 if inject is None else inject.numel()
    for attempt in range(8):         # each overflow learns the exact rates: one re-run is the rule
        cap = arena.caps(L)
        cap["ver"] += ninj
        early_done = None
        if early is not None:            # prefilter already queued (behind the line index)
            cap["gram"] = early.cap
            gh, cnt = early.gh, early.cnt
            early_done = early.done
        else:
            gh = torch.empty(cap["gram"], dtype=torch.int64, device=dev)
            # [gram hits, candidates, verified hits] then [unique hits, events] (post_hits counters),
            # then the events that fit their buffer (deferred steps: post_events' ne_fit) and the
            # DP step's overflow veto (k_dp_carry)
            cnt = torch.zeros(7, dtype=torch.int64, device=dev)
        cand = torch.empty(cap["cand"], dtype=torch.int64, device=dev)
        ver = torch.empty(cap["ver"], dtype=torch.int64, device=dev)
        c0 = cnt.data_ptr()
        sst = st
        if side is not None and scans and tick is None:
            side[1].record()
            side[0].wait_event(side[1])
            sst = side[0].cuda_stream
        blk = line_block_index(line_start, nbytes)
        # the long pole first: literal-free scans (own stream when `side`)
        for sp in tabs["scan_passes"]:
            N.scan_multi(text.data_ptr(), nbytes, line_start.data_ptr(), line_len.data_ptr(), L, sp, ver.data_ptr(),
                         cap["ver"], c0 + 16, scan_grid(sp), sst, True)
        if tabs["scan_regs"].numel():
            N.scan_dev(text.data_ptr(), line_start.data_ptr(), line_len.data_ptr(), L, tabs["scan_regs"].data_ptr(),
                       tabs["scan_regs"].numel(), tabs["dfa"], ver.data_ptr(), cap["ver"], c0 + 16, sst)
        for ncls, glist in tabs["nfa_scan_lists"].items():
            if glist.numel():
                N.nfa(tabs["nfa_tables"].data_ptr(), glist.data_ptr(), glist.numel(), ncls, 0, L, text.data_ptr(),
                      line_start.data_ptr(), line_len.data_ptr(), 0, ver.data_ptr(), cap["ver"], c0 + 16, sst, True)
        if host_side is not None:          # region B: the scans' relaxation keys leave as the scans end
            host_side[0].begin(host_side[1])
            host_side[0].export_scan(ver, c0 + 16, cap["ver"], text, line_start, line_len, tabs["dfa"], sst)
        if sst != st:
            side[2].record(side[0])
        elif tick:
            tick("scan")
        if early is None:
            N.prefilter_dev(text.data_ptr(), nbytes, tabs["pf"], line_start.data_ptr(), L, gh.data_ptr(), cap["gram"],
                            c0, pf_grid, st)
        early = None                     # an overflow re-run launches everything itself
        if early_done is not None:       # the early prefilter ran on its own stream
            torch.cuda.current_stream(dev).wait_event(early_done)
        N.pf_verify_dev(gh.data_ptr(), cap["gram"], text.data_ptr(), nbytes, tabs["pf"], line_start.data_ptr(), L,
                        blk.data_ptr(), cand.data_ptr(), cap["cand"], c0 + 8, st, c0,
                        max(16, min(8192, nbytes >> 13)))
        if tick:
            tick("prefilter")
        if host_side is not None:          # region A: the prefilter candidates, right after the literal chain
            host_side[0].export_candidates(cand, c0 + 8, cap["cand"], text, line_start, line_len, tabs["dfa"], st)
        if sst != st:
            torch.cuda.current_stream(dev).wait_event(side[2])
        if host_side is not None:          # host backtracker answers for both regions -> append, all queued
            host_side[0].wait(ver, c0 + 16, cap["ver"], st)
        elif tabs.get("host_dev"):         # relaxation keys of regexes the host side path decided
            N.take_host(cand.data_ptr(), c0 + 8, cap["cand"], ver.data_ptr(), c0 + 16, cap["ver"], text.data_ptr(),
                        line_start.data_ptr(), line_len.data_ptr(), tabs["dfa"], None, st)
        if ninj:                           # (after the take: these keys are decided, never dropped)
            N.append_keys(ver.data_ptr(), cap["ver"], c0 + 16, inject.data_ptr(), ninj, st)
        n = cap["cand"] + cap["ver"]
        hits = torch.empty(n, dtype=torch.int64, device=dev)
        hit_line = torch.empty(n, dtype=torch.int32, device=dev)
        hit_off = torch.empty(R + 1, dtype=torch.int64, device=dev)
        ev_cnt = torch.empty(n, dtype=torch.int64, device=dev)
        ev_end = torch.empty(n, dtype=torch.int64, device=dev)

        def call(wp, wn):
            return N.post_hits(cand.data_ptr(), n, cap["cand"], lbits, rbits, R, text.data_ptr(),
                               line_start.data_ptr(), line_len.data_ptr(), tabs["dfa"], evt, hits.data_ptr(),
                               hit_line.data_ptr(), hit_off.data_ptr(), ev_cnt.data_ptr(), ev_end.data_ptr(),
                               c0 + 24, wp, wn, st, True, ver.data_ptr(), c0 + 8)

        _run_ws(call, ws)
        if defer:
            return hits, hit_line, hit_off, ev_cnt, ev_end, n, cnt, cap
        g, k, v, nh, ne = cnt[:5].tolist()             # the one host read
        arena.last = {"lines": L, "gram_hits": g, "prefilter_candidates": k, "scan_hits": v, "hits": nh, "events": ne}
        ok = g <= cap["gram"] and k <= cap["cand"] and v <= cap["ver"]
        arena.learn(L, {"gram": g, "cand": k, "ver": v}, overflow=not ok)
        if ok:
            return hits[:nh], hit_line, hit_off, ev_cnt, ev_end, nh, ne
        if host_side is not None:          # the worker answers every job before the re-run's export
            if host_side[0].settle() == 1:  # the GPU stopped waiting: the caller re-runs host-verified
                raise SidePathTimeout()
    raise RuntimeError(f"matching: buffers still overflowing after 8 attempts ({arena.last})")


class SidePathTimeout(RuntimeError):
    """The GPU's wait for the backtracker side path's host answer timed out (ops/side_path.py):
    the batch re-runs on the host-verified path (``Engine.prepare``)."""


def results_buffer(ne: int, nkeys: int, device) -> torch.Tensor:
    """One device buffer for everything a batch returns to the host (one D2H, no cat):
    [score f64 x ne | frequency counts i64 x max(nkeys, 1) | line i32 x ne | pattern i32 x ne |
    segment i32 x ne]."""
    return torch.empty(20 * ne + 8 * max(nkeys, 1), dtype=torch.uint8, device=device)


def results_views(buf: torch.Tensor, ne: int, nkeys: int):
    """(score, freq_counts, ev_line, ev_pat, ev_seg) views of ``results_buffer``."""
    k = max(nkeys, 1)
    a, b = 8 * ne, 8 * ne + 8 * k
    return (buf[:a].view(torch.float64), buf[a:b].view(torch.int64), buf[b:b + 4 * ne].view(torch.int32),
            buf[b + 4 * ne:b + 8 * ne].view(torch.int32), buf[b + 8 * ne:b + 12 * ne].view(torch.int32))


def post_events(hits, nh: int, ev_cnt, ev_end, ne: int, L: int, evt: tuple, text, line_start, line_len, dfa_tuple,
                nkeys: int, ws: Optional[Workspace], features: bool = True, ctx_ext: Tuple[int, int] = (1 << 30, 1 << 30),
                out: Optional[torch.Tensor] = None, dcounts: Optional[torch.Tensor] = None,
                ne_fit: Optional[torch.Tensor] = None):
    """Events in reference order + segment, frequency rank/key, per-key counts and context features
    (or, with ``features=False``, the int32 window coverage per line for another feature engine).
    ``ctx_ext`` = table extents of the 4 context DFAs (trans, acc entries) for LDS staging.
    ``out``: a ``results_buffer`` receiving line / pattern / segment / frequency counts.
    ``dcounts``: device [hits, events] counts (device only); nh / ne are then capacities and the
    outputs are left unset when the events exceed ne (the caller re-runs). ``ne_fit`` (int64[1],
    with ``dcounts``): receives the event count, or 0 when the events did not fit -- the count the
    batch's later kernels must read (score, summary), so they never touch unset event fields."""
    dev = text.device
    if out is not None:
        _, freq_counts, ev_line, ev_pat, ev_seg = results_views(out, ne, nkeys)
    else:
        ev_line = torch.empty(ne, dtype=torch.int32, device=dev)
        ev_pat = torch.empty(ne, dtype=torch.int32, device=dev)
        ev_seg = torch.empty(ne, dtype=torch.int32, device=dev)
        freq_counts = (torch.empty if nkeys else torch.zeros)(max(nkeys, 1), dtype=torch.int64, device=dev)
    ev_rank = torch.empty(ne, dtype=torch.int64, device=dev)
    ev_fkey = torch.empty(ne, dtype=torch.int64, device=dev)
    if out is not None and not nkeys:
        freq_counts.zero_()
    # k_feat_cov writes every line (0 outside windows); the host twin too
    feat = torch.empty(max(L, 1), dtype=torch.uint8, device=dev) if features and L else \
        torch.zeros(max(L, 1), dtype=torch.uint8, device=dev)
    cov = None if features else torch.zeros(max(L, 1), dtype=torch.int32, device=dev)
    lbits = N.bits_for(max(L, 1))

    def call(wp, wn):
        return N.post_events(hits.data_ptr() if nh else 0, nh, ev_cnt.data_ptr(), ev_end.data_ptr(), ne, L, lbits,
                             evt, text.data_ptr(), line_start.data_ptr(), line_len.data_ptr(), dfa_tuple,
                             ev_line.data_ptr(), ev_pat.data_ptr(), ev_seg.data_ptr(), ev_rank.data_ptr(),
                             ev_fkey.data_ptr(), freq_counts.data_ptr(), feat.data_ptr() if features else 0,
                             _p(cov), ctx_ext[0], ctx_ext[1], wp, wn, _s(text), text.is_cuda, _p(dcounts),
                             _p(ne_fit))

    if text.is_cuda:
        _run_ws(call, ws)
    else:
        call(0, 0)
    return ev_line, ev_pat, ev_seg, ev_rank, ev_fkey, freq_counts, feat, cov


SUMMARY_MAX_K = 1024


def _check_k(k: int) -> None:
    """The summary kernel keeps at most SUMMARY_MAX_K rows: a larger top-k is a configuration
    error, not something to truncate silently (engine.topk is validated at config load)."""
    if int(k) > SUMMARY_MAX_K:
        raise ValueError(f"top-k {k} exceeds the summary kernel's maximum of {SUMMARY_MAX_K}")


def summarize(score: torch.Tensor, pat: torch.Tensor, line: torch.Tensor, k: int, sev_index: torch.Tensor,
              npat: int, nsev: int, line_add: Optional[torch.Tensor] = None, ws: Optional[Workspace] = None,
              pack_events: bool = False, hist_out: Optional[torch.Tensor] = None,
              rows_out: Optional[torch.Tensor] = None, dn: Optional[torch.Tensor] = None):
    """Top-k rows + histograms of scored events (csrc/kernels/summarize.hip).

    ``line`` is int32 (local, plus the device scalar ``line_add``) or int64 (global);
    ``sev_index[p]`` is pattern p's index into the library's distinct severity names. Returns
    (rows float64[k, 3] = (score, global line, pattern) ordered score desc, line asc, pattern asc,
    missing rows = (-inf, -1, -1); pat_hist int64[npat]; sev_hist int64[nsev]; packed) where
    ``packed`` (with ``pack_events``) is every event as uint8[20 n] = [global line int64 x n |
    score f64 x n | pattern int32 x n], written by the same kernel. No host sync. ``dn``: device
    event count (the arrays are capacities; ``packed`` then holds the events at stride *dn)."""
    dev = score.device
    _check_k(k)
    k = max(1, int(k))
    n = score.numel()
    rows = rows_out if rows_out is not None else torch.empty((k, 3), dtype=torch.float64, device=dev)
    if hist_out is not None:           # zeroed by the caller: [pattern hist | severity hist | ...]
        pat_hist, sev_hist = hist_out[:npat], hist_out[npat:npat + nsev]
    else:
        hist = torch.zeros(npat + nsev + 1, dtype=torch.int64, device=dev)
        pat_hist, sev_hist = hist[:npat], hist[npat:npat + nsev]
    packed = torch.empty(20 * n, dtype=torch.uint8, device=dev) if pack_events else None
    sev_of_pat = sev_index
    l32 = line.data_ptr() if line.dtype == torch.int32 else 0
    l64 = line.data_ptr() if line.dtype == torch.int64 else 0
    ins = (score.data_ptr() if n else 0, pat.data_ptr() if n else 0, l32 if n else 0, l64 if n else 0,
           _p(line_add), sev_of_pat.data_ptr(), 0, _p(packed) if n else 0, _p(dn))

    def call(wp, wn):
        return N.summarize(ins, n, k, nsev, rows.data_ptr(), pat_hist.data_ptr(), sev_hist.data_ptr(), wp, wn, _s(score),
                           score.is_cuda)

    if score.is_cuda:
        _run_ws(call, ws if ws is not None else Workspace(dev))
    else:
        call(0, 0)
    return rows, pat_hist[:npat], sev_hist[:nsev], packed


def dp_payload_width(nk: int, ns: int) -> int:
    """Columns of the C1+C3+C4 all-gather payload: owned lines, nk counts, ns chain slots, overflow."""
    return 1 + nk + ns + 1


def dp_pack(own_lines: int, freq_counts: torch.Tensor, nk: int, chain: torch.Tensor,
            out: Optional[torch.Tensor] = None, overflow: Optional[tuple] = None) -> torch.Tensor:
    """C1+C3+C4 all-gather payload [owned lines | nk frequency counts | chain table | overflow flag]
    (int64); ``out``: where to write it (this rank's row of an in-place all-gather buffer);
    ``overflow`` = (device counters [5], host capacities [4]) of a deferred-count step: the flag is
    set when a counter exceeded its buffer (every rank then vetoes the step's record and re-runs)."""
    ns = chain.numel()
    pack = out if out is not None else torch.empty(dp_payload_width(nk, ns), dtype=torch.int64, device=chain.device)
    fc = freq_counts if freq_counts.dtype == torch.int64 else freq_counts.to(torch.int64)
    cnt, caps = (overflow[0].data_ptr(), [int(c) for c in overflow[1]]) if overflow is not None else (0, [])
    N.dp_pack(int(own_lines), fc.data_ptr(), nk, chain.data_ptr(), ns, pack.data_ptr(), _s(chain), chain.is_cuda,
              cnt, caps)
    return pack


def dp_carry(g: torch.Tensor, rank: int, nk: int, ns: int, halo_left: int, tot: Optional[torch.Tensor],
             slot_e0: torch.Tensor, slot_k: torch.Tensor, red_tail: Optional[torch.Tensor] = None,
             veto_out: Optional[torch.Tensor] = None, zero: Optional[torch.Tensor] = None,
             stream: Optional[tuple] = None):
    """From the gathered payloads: (own_start[1], g0[1], n[1], carry[nk], seq_carry uint8[ns],
    veto[1]); ``red_tail`` (optional) receives this rank's frequency counts; veto = any rank's
    overflow flag (written into ``veto_out`` when given); ``zero`` (int64, optional) is zeroed by
    the same kernel. ``stream`` = (seq_base uint8[ns], line_base, n_fixed, seq_next uint8[ns]): one
    step of a stream of steps (the earlier steps' sequence state and line count, an open N, and the
    sequence state after this step written into seq_next)."""
    dev = g.device
    sc = torch.empty(5, dtype=torch.int64, device=dev)          # own_start, g0, n, veto (+ pad)
    carry = torch.empty(max(nk, 1), dtype=torch.int64, device=dev)
    if nk == 0:
        carry.zero_()
    seq = torch.empty(max(ns, 1), dtype=torch.uint8, device=dev)
    g = g.contiguous()
    p = sc.data_ptr()
    veto = veto_out if veto_out is not None else sc[3:4]
    args = (g.data_ptr(), g.shape[0], rank, nk, ns, int(halo_left), _p(tot) if nk else 0, slot_e0.data_ptr(),
            slot_k.data_ptr(), p, p + 8, p + 16, carry.data_ptr(), seq.data_ptr(), _p(red_tail), veto.data_ptr(),
            _p(zero), 0 if zero is None else zero.numel())
    if stream is not None:
        sb, lb, nf, sn = stream
        args = args + (_p(sb), int(lb), int(nf), _p(sn))
    N.dp_carry(args, _s(g), g.is_cuda)
    return sc[0:1], sc[1:2], sc[2:3], carry, seq, veto


def topk_rows(rows: torch.Tensor, k: int, ws: Optional[Workspace] = None) -> torch.Tensor:
    """Merge (score, line, pattern) rows (e.g. every rank's top-k) into the k best, same order."""
    dev = rows.device
    _check_k(k)
    k = max(1, int(k))
    rows = rows.contiguous()
    out = torch.empty((k, 3), dtype=torch.float64, device=dev)
    ins = (0, 0, 0, 0, 0, 0, rows.data_ptr())

    def call(wp, wn):
        return N.summarize(ins, rows.shape[0], k, 0, out.data_ptr(), 0, 0, wp, wn, _s(rows), rows.is_cuda)

    if rows.is_cuda:
        _run_ws(call, ws if ws is not None else Workspace(dev))
    else:
        call(0, 0)
    return out


def rescore(gl: torch.Tensor, fac: torch.Tensor, n_lines: int, sp_tuple) -> torch.Tensor:
    """Final streaming scores: the score kernel's kept factors with the chronological factor of the
    true global line count (left-to-right product, ScoringService.java:102-109)."""
    n = gl.numel()
    out = torch.empty(n, dtype=torch.float64, device=gl.device)
    if n:
        N.rescore(gl.data_ptr(), fac.contiguous().data_ptr(), n, int(n_lines), sp_tuple, out.data_ptr(), _s(gl),
                  gl.is_cuda)
    return out


def score_fused(ev_line, ev_pat, ev_seg, ev_rank, ev_fkey, freq_carry, st_tuple, sp_tuple, with_factors=False,
                out: Optional[torch.Tensor] = None, dn: Optional[torch.Tensor] = None):
    """k_score with the frequency count fused in: freq = carry[fkey] + rank (-1 without a key).
    ``out``: float64[n] destination (e.g. the score view of a ``results_buffer``); ``dn``: device
    event count (the arrays are then capacities; device only)."""
    n = ev_line.numel()
    if out is None:
        out = torch.empty(n, dtype=torch.float64, device=ev_line.device)
    fac = torch.empty((n, 7), dtype=torch.float64, device=ev_line.device) if with_factors else None
    if n == 0:
        return out, fac
    args = (ev_line.data_ptr(), ev_pat.data_ptr(), ev_seg.data_ptr(), ev_rank.data_ptr(), ev_fkey.data_ptr(),
            freq_carry.data_ptr(), n, st_tuple, sp_tuple, out.data_ptr(), _p(fac))
    if ev_line.is_cuda:
        N.score_dev(*args, _s(ev_line), _p(dn))
    else:
        N.score_host(*args)
    return out, fac


# ---------------------------------------------------------------------------------------------
# coverage-gap report (csrc/kernels/gaps.hip): features of every line, template signatures

SIG_MAX_BYTES = 1024    # a line's template covers its first KiB (csrc/kernels/gaps_core.h)


def context_features_all(text, line_start, line_len, dfa_tuple,
                         ctx_ext: Tuple[int, int] = (1 << 30, 1 << 30)) -> torch.Tensor:
    """Context features of EVERY line (uint8[L]; bit0 ERROR, bit1 WARN when not ERROR, bit2 stack
    frame, bit3 exception / error class name): k_feat_cov without a coverage filter."""
    L = line_start.numel()
    feat = torch.empty(L, dtype=torch.uint8, device=text.device)
    if L == 0:
        return feat
    if text.is_cuda:
        N.feat_all_dev(L, text.data_ptr(), line_start.data_ptr(), line_len.data_ptr(), dfa_tuple, ctx_ext[0],
                       ctx_ext[1], feat.data_ptr(), _s(text))
    else:
        N.feat_all_host(L, text.data_ptr(), line_start.data_ptr(), line_len.data_ptr(), dfa_tuple, feat.data_ptr())
    return feat


def _gap_sig(text, line_start, line_len, feat, cov, sel, every: bool, cap: int):
    """k_gap_sig / its host twin with the capacity protocol of ``scan``: (line, sig, candidates,
    selected), one read of the two counters per run."""
    dev = text.device
    L = line_start.numel()
    if sel is not None:
        sel = sel.to(device=dev, dtype=torch.int32).contiguous()
    while True:
        out_line = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
        out_sig = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
        cnt = torch.zeros(2, dtype=torch.int64, device=dev)
        N.gap_sig(text.data_ptr(), text.numel(), line_start.data_ptr(), line_len.data_ptr(), L, _p(feat), _p(cov),
                  _p(sel), 0 if sel is None else sel.numel(), every, out_line.data_ptr(), out_sig.data_ptr(), cap,
                  cnt.data_ptr(), _s(text), text.is_cuda)
        n_cand, n = cnt.tolist()
        if n <= cap:
            return out_line[:n], out_sig[:n], n_cand
        cap = n


def line_signatures(text, line_start, line_len, sel: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Template signatures (int64 bit patterns of FNV-1a-64, ``golden.line_signature``) of the
    lines ``sel`` (int32, any order, repeats allowed), or of every line."""
    n = line_start.numel() if sel is None else sel.numel()
    if n == 0:
        return torch.empty(0, dtype=torch.int64, device=text.device)
    return _gap_sig(text, line_start, line_len, None, None, sel, sel is None, n)[1]


def gap_lines(text, line_start, line_len, feat: torch.Tensor, cov: Optional[torch.Tensor],
              cap: int) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """The candidate lines of ``feat`` (uint8[L], every line's context features) that ``cov``
    (uint8[L], or None: nothing covered) does not cover: (line int32[n], signature int64[n],
    number of candidates). GPU: the pairs come in no particular order; CPU: in line order."""
    if line_start.numel() == 0:
        return (torch.empty(0, dtype=torch.int32, device=text.device),
                torch.empty(0, dtype=torch.int64, device=text.device), 0)
    if feat.dtype != torch.uint8 or feat.numel() < line_start.numel() or not feat.is_contiguous():
        raise ValueError("gap_lines: feat must be contiguous uint8[L]")
    if cov is not None and (cov.dtype != torch.uint8 or cov.numel() < line_start.numel() or not cov.is_contiguous()):
        raise ValueError("gap_lines: cov must be contiguous uint8[L]")
    return _gap_sig(text, line_start, line_len, feat, cov, None, False, cap)


# ---------------------------------------------------------------------------------------------
# signature group table (csrc/kernels/gap_table.hip): the report's grouping across launches

GT_EMPTY = -(1 << 63)       # empty marker of the key column (csrc/kernels/gap_table.h)
GT_TILE = 2048              # pairs per block of k_gap_fold at most (small launches get smaller tiles)
GT_LDS_SLOTS = 1024         # slots of its LDS table: more distinct signatures in a tile go to HBM directly
I64_MAX = (1 << 63) - 1


class _SlotTable:
    """What the device-resident hash tables share: the validation of ``cap`` / ``tile``, the
    slot counter, the capacity rule with its growth, and the rows. A subclass has its columns
    (``_alloc``, ``_tab``, ``_row_dtypes``), the names of its native calls and its ``fold``.

    Capacity: before ``n`` entries are folded, ``2 * (used + n) <= cap`` holds -- the table grows
    (rows of the old one re-inserted into one at least twice as large) when it does not. ``used``
    is bounded on the host by the number of entries folded so far; the device counter is read only
    when that bound crosses the limit, so steady folding reads nothing of the table."""

    _max_tile: int
    _row_dtypes: tuple
    _rows_op: str
    _reinsert_op: str

    def __init__(self, device, cap: int = 1 << 12, tile: int = 0):
        cap, name = max(2, int(cap)), type(self).__name__
        self.tile = int(tile)
        if self.tile and (self.tile < 256 or self.tile > self._max_tile or self.tile % 256):
            raise ValueError("%s: tile must be 256..%d, a multiple of 256" % (name, self._max_tile))
        if cap & (cap - 1):
            raise ValueError("%s: cap must be a power of two" % name)
        self.device = torch.device(device)
        self._bound = 0             # host upper bound of the occupied slots
        self._alloc(cap)

    @property
    def _cuda(self) -> bool:
        return self.device.type == "cuda"

    @property
    def used(self) -> int:
        """Occupied slots (a read of the device counter)."""
        used, lost = self._used.tolist()
        if lost:
            raise RuntimeError("%s: %d entries found no slot (capacity rule broken)" % (type(self).__name__, lost))
        self._bound = used
        return used

    def _rows(self, n: int):
        """Every column of the ``n`` occupied slots, in no particular order."""
        cols = tuple(torch.empty(n, dtype=t, device=self.device) for t in self._row_dtypes)
        cnt = torch.zeros(1, dtype=torch.int64, device=self.device)
        getattr(N, self._rows_op)(self._tab(), tuple(c.data_ptr() for c in cols), n, cnt.data_ptr(), _s(self._key),
                                  self._cuda)
        if int(cnt.item()) != n:
            raise RuntimeError("%s: %d occupied slots, the counter says %d" % (type(self).__name__, int(cnt.item()), n))
        return cols

    def _reinsert(self, rows, n: int) -> None:
        """``n`` rows of distinct keys into the (empty) table."""
        if n:
            getattr(N, self._reinsert_op)(self._tab(), tuple(c.data_ptr() for c in rows), n, _s(self._key), self._cuda)
            self._used[0] = n

    @staticmethod
    def _fit(cap: int, used: int, n: int) -> int:
        while 2 * (used + n) > cap:
            cap *= 2
        return cap

    def _reserve(self, n: int) -> None:
        """The capacity rule, before ``n`` entries are folded."""
        if 2 * (self._bound + n) > self.cap:
            used = self.used                                    # the bound crossed the limit: the real count
            cap = self._fit(self.cap, used, n)
            if cap != self.cap:
                rows = self._rows(used)
                self._alloc(cap)
                self._reinsert(rows, used)
        self._bound += n


class GapTable(_SlotTable):
    """Device-resident groups of (signature, ordinal) pairs: per signature its count, its smallest
    ordinal and the number of documents it occurs in, kept across ``fold`` calls (the chunks of a
    stream, the documents of a corpus). GPU: k_gap_fold / k_gap_winners / k_gap_rows; CPU: their
    host twins on the same layout. Capacity and growth: ``_SlotTable``; steady folding reads
    nothing but the winners' count."""

    _max_tile = GT_TILE
    _row_dtypes = (torch.int64, torch.int64, torch.int64, torch.int32, torch.int32)
    _rows_op, _reinsert_op = "gap_rows", "gap_reinsert"

    def __init__(self, device, cap: int = 1 << 12, tile: int = 0):
        """``tile``: pairs per block of k_gap_fold (256..GT_TILE, a multiple of 256) instead of the
        size the launch picks from its number of pairs (tests: the paths of a full-size tile
        without millions of pairs)."""
        super().__init__(device, cap, tile)
        self._last_doc = -1

    def _alloc(self, cap: int) -> None:
        dev = self.device
        self.cap = cap
        self._key = torch.full((cap + 1,), GT_EMPTY, dtype=torch.int64, device=dev)
        self._key[cap] = 0          # the side slot of the signature that equals the marker: unclaimed
        self._count = torch.zeros(cap + 1, dtype=torch.int64, device=dev)
        self._first = torch.full((cap + 1,), I64_MAX, dtype=torch.int64, device=dev)
        self._docs = torch.zeros(cap + 1, dtype=torch.int32, device=dev)
        self._last = torch.full((cap + 1,), -1, dtype=torch.int32, device=dev)
        self._used = torch.zeros(2, dtype=torch.int64, device=dev)

    def _tab(self):
        return (self._key.data_ptr(), self._count.data_ptr(), self._first.data_ptr(), self._docs.data_ptr(),
                self._last.data_ptr(), self._used.data_ptr(), self.cap)

    def rows(self) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """(signature int64, count int64, smallest ordinal int64, documents int32) of every group,
        in no particular order."""
        return self._rows(self.used)[:4]

    def sorted_rows(self) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(signature, count, smallest ordinal) of every group, by signature (as a signed number)."""
        key, count, first, _ = self.rows()
        key, o = torch.sort(key)
        return key, count[o], first[o]

    def lookup(self, key: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, int]:
        """The join of ``key`` (int64[n], on the table's device) with the groups: (count, smallest
        ordinal, found) per key -- 0, 0 and False for a key the table does not hold -- and the
        number of groups of the table. One ``rows``; what a missing key means is the caller's."""
        t_key, t_count, t_first = self.sorted_rows()
        groups = t_key.numel()
        if groups == 0:
            return torch.zeros_like(key), torch.zeros_like(key), torch.zeros_like(key, dtype=torch.bool), 0
        pos = torch.searchsorted(t_key, key).clamp(max=groups - 1)
        found = t_key[pos] == key
        return torch.where(found, t_count[pos], 0), torch.where(found, t_first[pos], 0), found, groups

    def fold(self, sig: torch.Tensor, ord: torch.Tensor, doc: int = 0, winners: bool = True) -> torch.Tensor:
        """Fold the pairs (sig[i], ord[i]) of document ``doc`` (one document per call, numbers never
        decreasing) into the table. Returns the indices (int64, no particular order) of the pairs
        that hold their group's smallest ordinal after this call -- or, with ``winners=False``
        (a caller that keeps no examples), nothing: k_gap_winners and the read of its count are
        left out."""
        n = sig.numel()
        if ord.numel() != n:
            raise ValueError("GapTable.fold: sig and ord differ in length")
        doc = int(doc)
        if doc < self._last_doc or not 0 <= doc < (1 << 31):
            raise ValueError("GapTable.fold: document numbers must not decrease")
        if n == 0:
            return torch.empty(0, dtype=torch.int64, device=self.device)
        sig = sig.to(device=self.device, dtype=torch.int64).contiguous()
        ord = ord.to(device=self.device, dtype=torch.int64).contiguous()
        self._reserve(n)
        self._last_doc = doc
        tab, st = self._tab(), _s(self._key)
        N.gap_fold(tab, sig.data_ptr(), ord.data_ptr(), n, doc, st, self._cuda, self.tile)
        if not winners:
            return torch.empty(0, dtype=torch.int64, device=self.device)
        out = torch.empty(n, dtype=torch.int64, device=self.device)
        cnt = torch.zeros(1, dtype=torch.int64, device=self.device)
        N.gap_winners(tab, sig.data_ptr(), ord.data_ptr(), n, out.data_ptr(), cnt.data_ptr(), st, self._cuda)
        return out[:int(cnt.item())]

    def contains(self, sig: torch.Tensor) -> torch.Tensor:
        """bool[n]: the table holds sig[i] (k_gap_contains or its host twin)."""
        sig = sig.to(device=self.device, dtype=torch.int64).contiguous()
        out = torch.empty(sig.numel(), dtype=torch.uint8, device=self.device)
        if sig.numel():
            N.gap_contains(self._tab(), sig.data_ptr(), sig.numel(), out.data_ptr(), _s(self._key), self._cuda)
        return out.bool()

    @classmethod
    def from_signatures(cls, device, sig: torch.Tensor, cap: Optional[int] = None) -> "GapTable":
        """A table that holds exactly the DISTINCT signatures ``sig`` (count 1 each, first ordinal
        0), built with k_gap_reinsert. ``cap``: a capacity of its own (a power of two >= n; tests:
        a full table, wrap-around probing) instead of the smallest that keeps the table at most
        half full. ValueError on duplicates."""
        sig = sig.to(device=torch.device(device), dtype=torch.int64).contiguous()
        n = sig.numel()
        if n and torch.unique(sig).numel() != n:
            raise ValueError("GapTable.from_signatures: duplicate signatures")
        if cap is None:
            cap = cls._fit(1 << 12, 0, n)
        elif cap < n:
            raise ValueError("GapTable.from_signatures: cap below the number of signatures")
        tab = cls(device, cap=cap)
        if n:
            dev = tab.device
            tab._reinsert((sig, torch.ones(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev),
                           torch.ones(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)), n)
            tab._bound = n
            tab._last_doc = 0
        return tab


# ---------------------------------------------------------------------------------------------
# cell table of the trends report (csrc/kernels/trends.hip, cell_table.h)

CT_UNDATED = -(1 << 63)     # the bucket of lines without an effective time
CT_TILE = 2048              # lines per block of k_cell_fold at most
CT_LDS_SLOTS = 1024         # slots of its LDS table: more distinct cells in a tile go to HBM directly


class CellTable(_SlotTable):
    """Device-resident counts per cell (template signature, time bucket): per cell its lines and
    its smallest global line number, kept across ``fold`` calls (the chunks of a stream). The key
    column holds ``golden.trend_cell_key(sig, bucket)``. GPU: k_cell_fold / k_cell_rows /
    k_cell_reinsert; CPU: their host twins on the same layout. Capacity and growth: ``_SlotTable``.
    ``tile``: lines per block of k_cell_fold (256..CT_TILE, a multiple of 256) instead of the size
    the launch picks from its number of lines (tests)."""

    _max_tile = CT_TILE
    _row_dtypes = (torch.int64,) * 4
    _rows_op, _reinsert_op = "cell_rows", "cell_reinsert"

    def _alloc(self, cap: int) -> None:
        dev = self.device
        self.cap = cap
        self._key = torch.full((cap + 1,), GT_EMPTY, dtype=torch.int64, device=dev)
        self._key[cap] = 0          # the side slot of the cell whose key equals the marker: unclaimed
        self._sig = torch.zeros(cap + 1, dtype=torch.int64, device=dev)
        self._bucket = torch.zeros(cap + 1, dtype=torch.int64, device=dev)
        self._count = torch.zeros(cap + 1, dtype=torch.int64, device=dev)
        self._first = torch.full((cap + 1,), I64_MAX, dtype=torch.int64, device=dev)
        self._used = torch.zeros(2, dtype=torch.int64, device=dev)

    def _tab(self):
        return (self._key.data_ptr(), self._sig.data_ptr(), self._bucket.data_ptr(), self._count.data_ptr(),
                self._first.data_ptr(), self._used.data_ptr(), self.cap)

    def rows(self) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """(signature, bucket, lines, smallest line) of every cell, int64 each, in no particular
        order; the bucket of a template's undated lines is ``CT_UNDATED``."""
        return self._rows(self.used)

    def fold(self, sig: torch.Tensor, eff: torch.Tensor, line_base: int, W: int) -> None:
        """Fold n consecutive lines into the table: line i has the signature ``sig[i]``, the
        effective time ``eff[i]`` (``TS_NONE``: undated) and the global number ``line_base + i``;
        its cell is (sig[i], floor(eff[i] / W))."""
        n = sig.numel()
        if eff.numel() != n:
            raise ValueError("CellTable.fold: sig and eff differ in length")
        if isinstance(W, bool) or int(W) < 1:
            raise ValueError("CellTable.fold: W must be >= 1")
        if not 0 <= int(line_base) <= I64_MAX - n:
            raise ValueError("CellTable.fold: line_base out of range")
        if n == 0:
            return
        sig = sig.to(device=self.device, dtype=torch.int64).contiguous()
        eff = eff.to(device=self.device, dtype=torch.int64).contiguous()
        self._reserve(n)
        N.cell_fold(self._tab(), sig.data_ptr(), eff.data_ptr(), n, int(line_base), int(W), _s(self._key), self._cuda,
                    self.tile)


# ---------------------------------------------------------------------------------------------
# novelty report (csrc/kernels/novelty.hip): the lines whose template a baseline table does not hold

NV_MAX_LINES = 2048         # lines per block of k_novel_sig at most
NV_CAND, NV_EVENT = 1, 2    # flag bits of a novel line: gap candidate, an event lies on it


def novel_lines(text, line_start, line_len, table: GapTable, feat: Optional[torch.Tensor] = None,
                ev_mask: Optional[torch.Tensor] = None, cap: Optional[int] = None, per_block: int = 0):
    """Every line whose template signature ``table`` does not hold: (line int32[n], signature
    int64[n], flag uint8[n], (candidates among all lines, novel lines, novel candidates)). Flag
    bit0: the line is a gap candidate of ``feat`` (uint8[L] context features; None: no candidates),
    bit1: ``ev_mask`` (uint8[L]; None: no events) is set. One pass over the text (k_novel_sig) with
    the capacity protocol of ``gap_lines``; ``cap=None`` starts well below L -- a mostly healthy
    log has few novel lines. ``per_block``: lines per block instead of the size the launch picks
    (tests). GPU: the triples come in no particular order; CPU: in line order."""
    dev = text.device
    L = line_start.numel()
    if table.device != dev:
        raise ValueError("novel_lines: the table lives on %s, the text on %s" % (table.device, dev))
    for name, m in (("feat", feat), ("ev_mask", ev_mask)):
        if m is not None and (m.dtype != torch.uint8 or m.numel() < L or not m.is_contiguous() or m.device != dev):
            raise ValueError("novel_lines: %s must be contiguous uint8[L] on the text's device" % name)
    if per_block and not 0 < per_block <= NV_MAX_LINES:
        raise ValueError("novel_lines: per_block must be 1..%d" % NV_MAX_LINES)
    if L == 0:
        return (torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int64, device=dev),
                torch.empty(0, dtype=torch.uint8, device=dev), (0, 0, 0))
    cap = max(1024, L // 16) if cap is None else max(0, int(cap))
    while True:
        out_line = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
        out_sig = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
        out_flag = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
        cnt = torch.zeros(3, dtype=torch.int64, device=dev)
        N.novel_sig(text.data_ptr(), text.numel(), line_start.data_ptr(), line_len.data_ptr(), L, table._tab(),
                    _p(feat), _p(ev_mask), out_line.data_ptr(), out_sig.data_ptr(), out_flag.data_ptr(), cap,
                    cnt.data_ptr(), _s(text), text.is_cuda, per_block)
        n_cand, n, n_ncand = cnt.tolist()
        if n <= cap:
            return out_line[:n], out_sig[:n], out_flag[:n], (n_cand, n, n_ncand)
        cap = n


# ---------------------------------------------------------------------------------------------
# lead-up report (csrc/kernels/leadup.hip): every line's signature, the lines shortly before an event

LD_MAX_LINES = 2048         # lines per block of k_lead_sig at most
LD_MAX_WINDOW = 4096        # lines before an event at most


def lead_lines(text, line_start, line_len, ev: Optional[torch.Tensor], window: int, cap: Optional[int] = None,
               per_block: int = 0):
    """The signature of every line, and the lines in the lead-up of an event: (sig int64[L], lead
    uint8[L], line int32[n], pair_sig int64[n], n). ``ev``: the lines that carry an event (int32,
    sorted and distinct, counted as the lines are; empty or None: no events). Line x is in the
    lead-up iff some e of ``ev`` has ``x < e <= x + window``; the n lead-up lines come again as
    (line, signature) pairs. One pass over the text (k_lead_sig) with the capacity protocol of
    ``novel_lines``; ``cap=None`` starts well below L -- the lead-up of a mostly healthy log is
    short. ``per_block``: lines per block instead of the size the launch picks (tests). GPU: the
    pairs come in no particular order; CPU: in line order."""
    dev = text.device
    L = line_start.numel()
    if not 1 <= window <= LD_MAX_WINDOW:
        raise ValueError("lead_lines: window must be 1..%d" % LD_MAX_WINDOW)
    if ev is not None and (ev.dtype != torch.int32 or ev.dim() != 1 or not ev.is_contiguous() or ev.device != dev):
        raise ValueError("lead_lines: ev must be contiguous int32[ne] on the text's device")
    if per_block and not 0 < per_block <= LD_MAX_LINES:
        raise ValueError("lead_lines: per_block must be 1..%d" % LD_MAX_LINES)
    sig = torch.empty(L, dtype=torch.int64, device=dev)
    lead = torch.empty(L, dtype=torch.uint8, device=dev)
    if L == 0:
        return (sig, lead, torch.empty(0, dtype=torch.int32, device=dev),
                torch.empty(0, dtype=torch.int64, device=dev), 0)
    ne = 0 if ev is None else ev.numel()
    cap = max(1024, L // 16) if cap is None else max(0, int(cap))
    while True:
        out_line = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
        out_sig = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
        cnt = torch.zeros(1, dtype=torch.int64, device=dev)
        N.lead_sig(text.data_ptr(), text.numel(), line_start.data_ptr(), line_len.data_ptr(), L,
                   _p(ev) if ne else 0, ne, int(window), sig.data_ptr(), lead.data_ptr(), out_line.data_ptr(),
                   out_sig.data_ptr(), cap, cnt.data_ptr(), _s(text), text.is_cuda, per_block)
        n = int(cnt.item())
        if n <= cap:
            return sig, lead, out_line[:n], out_sig[:n], n
        cap = n


# ---------------------------------------------------------------------------------------------
# correlation report (csrc/kernels/correlate.hip): the id-like tokens of lines as (line, key) pairs

KL_MAX_LINES = 2048         # lines per block of k_line_keys at most
KEY_MIN_LEN, KEY_MAX_LEN = 4, 64    # bounds of ``min_len``; the longest key token (csrc/kernels/key_core.h)
KEY_PER_LINE = 8            # distinct keys of a line at most


def line_keys(text, line_start, line_len, sel: Optional[torch.Tensor] = None, table: Optional[GapTable] = None,
              min_len: int = 8, cap: Optional[int] = None, per_block: int = 0):
    """The keys (``golden.line_keys``) of lines as pairs: (line int32[n], key int64[n], hit
    uint8[walked], (n, walked lines with at least one pair)). ``sel`` (int32, values in [0, L)):
    item i walks line ``sel[i]`` and ``hit[i]`` speaks of it; None: every line. ``table``: only
    the keys it holds are emitted (the filter comes after the line's first ``KEY_PER_LINE``
    distinct keys are chosen, so a line means the same in every pass). One pass over the text
    (k_line_keys) with the capacity protocol of ``lead_lines``. ``per_block``: lines per block
    instead of the size the launch picks (tests). GPU: the pairs come in no particular order;
    CPU: in item order, the keys of a line in byte order."""
    dev = text.device
    L = line_start.numel()
    if not KEY_MIN_LEN <= min_len <= KEY_MAX_LEN:
        raise ValueError("line_keys: min_len must be %d..%d" % (KEY_MIN_LEN, KEY_MAX_LEN))
    if sel is not None:
        if sel.dtype != torch.int32 or sel.dim() != 1 or not sel.is_contiguous() or sel.device != dev:
            raise ValueError("line_keys: sel must be contiguous int32[n] on the text's device")
        if sel.numel():
            lo, hi = torch.aminmax(sel)
            if int(lo) < 0 or int(hi) >= L:
                raise ValueError("line_keys: sel names a line outside [0, %d)" % L)
    if table is not None and table.device != dev:
        raise ValueError("line_keys: the table lives on %s, the text on %s" % (table.device, dev))
    if per_block and not 0 < per_block <= KL_MAX_LINES:
        raise ValueError("line_keys: per_block must be 1..%d" % KL_MAX_LINES)
    n = L if sel is None else sel.numel()
    hit = torch.empty(n, dtype=torch.uint8, device=dev)
    if n == 0:
        return (torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int64, device=dev), hit,
                (0, 0))
    # a re-run costs a whole pass over the text, a pair 12 bytes: start generously. Without a table a
    # line of a service log holds an id or two; with one, the event keys' lines are a fraction of the log
    cap = (max(1024, n // 4) if table is not None else max(1024, 2 * n)) if cap is None else max(0, int(cap))
    while True:
        out_line = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
        out_key = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
        cnt = torch.zeros(2, dtype=torch.int64, device=dev)
        N.line_keys(text.data_ptr(), text.numel(), line_start.data_ptr(), line_len.data_ptr(), L, _p(sel), n,
                    None if table is None else table._tab(), int(min_len), out_line.data_ptr(), out_key.data_ptr(),
                    hit.data_ptr(), cap, cnt.data_ptr(), _s(text), text.is_cuda, per_block)
        m, lines = cnt.tolist()
        if m <= cap:
            return out_line[:m], out_key[:m], hit, (m, lines)
        cap = m


# ---------------------------------------------------------------------------------------------
# values report (csrc/kernels/values.hip): template signature and numeric fields of every line

VL_MAX_LINES = 2048         # lines per block of k_line_vals at most
VAL_PER_LINE = 8            # fields of a line that count (csrc/kernels/val_core.h)


def line_values(text, line_start, line_len, cap: Optional[int] = None, per_block: int = 0):
    """Template signature and values (``golden.line_values``) of every line: (sig int64[L], line
    int32[n], key int64[n], value int32[n], (n, lines with at least one value)) -- a value of
    field j of line i is the triple (i, ``golden.val_key(sig[i], j)``, value). One pass over the
    text (k_line_vals) with the capacity protocol of ``line_keys``. ``per_block``: lines per block
    instead of the size the launch picks (tests). GPU: the triples come in no particular order;
    CPU: in line order, the fields of a line in byte order."""
    dev = text.device
    L = line_start.numel()
    if per_block and not 0 < per_block <= VL_MAX_LINES:
        raise ValueError("line_values: per_block must be 1..%d" % VL_MAX_LINES)
    sig = torch.empty(L, dtype=torch.int64, device=dev)
    if L == 0:
        return (sig, torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int64, device=dev),
                torch.empty(0, dtype=torch.int32, device=dev), (0, 0))
    # a re-run costs a whole pass over the text, a triple 16 bytes: a log line holds a number or two
    cap = max(1024, 2 * L) if cap is None else max(0, int(cap))
    while True:
        out_line = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
        out_key = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
        out_val = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
        cnt = torch.zeros(2, dtype=torch.int64, device=dev)
        N.line_vals(text.data_ptr(), text.numel(), line_start.data_ptr(), line_len.data_ptr(), L, sig.data_ptr(),
                    out_line.data_ptr(), out_key.data_ptr(), out_val.data_ptr(), cap, cnt.data_ptr(), _s(text),
                    text.is_cuda, per_block)
        m, lines = cnt.tolist()
        if m <= cap:
            return sig, out_line[:m], out_key[:m], out_val[:m], (m, lines)
        cap = m


# ---------------------------------------------------------------------------------------------
# variants report (csrc/kernels/variants.hip): template signature and token hashes of every line's
# fields, the value table (var_table.h)

VR_MAX_LINES = 2048         # lines per block of k_line_vars at most
VT_TILE = 2048              # triples per block of k_var_fold at most
VT_LDS_SLOTS = 1024         # slots of its LDS table: more distinct (field, value) in a tile go to HBM directly
CT_MIX = 0x9E3779B97F4A7C15  # cell_key(field, value) = field + value * CT_MIX mod 2^64 (cell_table.h)
I64_MIN = -(1 << 63)


def line_vars(text, line_start, line_len, cap: Optional[int] = None, per_block: int = 0):
    """Template signature and fields (``golden.line_fields``) of every line: (sig int64[L], line
    int32[n], field int64[n], value int64[n], (n, lines with at least one field)) -- field j of
    line i is the triple (i, ``golden.val_key(sig[i], j)``, ``golden.var_hash(token)``), whether
    or not the token reads as a number. One pass over the text (k_line_vars) with the capacity
    protocol of ``line_values``. ``per_block``: lines per block instead of the size the launch
    picks (tests). GPU: the triples come in no particular order; CPU: in line order, the fields
    of a line in byte order."""
    dev = text.device
    L = line_start.numel()
    if per_block and not 0 < per_block <= VR_MAX_LINES:
        raise ValueError("line_vars: per_block must be 1..%d" % VR_MAX_LINES)
    sig = torch.empty(L, dtype=torch.int64, device=dev)
    if L == 0:
        return (sig, torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int64, device=dev),
                torch.empty(0, dtype=torch.int64, device=dev), (0, 0))
    # a re-run costs a whole pass over the text, a triple 20 bytes: a log line holds a variable token or three
    cap = max(1024, 3 * L) if cap is None else max(0, int(cap))
    while True:
        out_line = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
        out_field = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
        out_value = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
        cnt = torch.zeros(2, dtype=torch.int64, device=dev)
        N.line_vars(text.data_ptr(), text.numel(), line_start.data_ptr(), line_len.data_ptr(), L, sig.data_ptr(),
                    out_line.data_ptr(), out_field.data_ptr(), out_value.data_ptr(), cap, cnt.data_ptr(), _s(text),
                    text.is_cuda, per_block)
        m, lines = cnt.tolist()
        if m <= cap:
            return sig, out_line[:m], out_field[:m], out_value[:m], (m, lines)
        cap = m


class VarTable(_SlotTable):
    """Device-resident counts per (field, value): per pair its triples, its smallest and its
    largest ordinal (global line numbers), kept across ``fold`` calls (the chunks of a stream).
    The key column holds ``cell_key(field, value)``; two pairs that share it are one entry. GPU:
    k_var_fold / k_var_rows / k_var_reinsert / k_var_winners; CPU: their host twins on the same
    layout. Capacity and growth: ``_SlotTable``. ``tile``: triples per block of k_var_fold
    (256..VT_TILE, a multiple of 256) instead of the size the launch picks (tests)."""

    _max_tile = VT_TILE
    _row_dtypes = (torch.int64,) * 5
    _rows_op, _reinsert_op = "var_rows", "var_reinsert"

    def _alloc(self, cap: int) -> None:
        dev = self.device
        self.cap = cap
        self._key = torch.full((cap + 1,), GT_EMPTY, dtype=torch.int64, device=dev)
        self._key[cap] = 0          # the side slot of the pair whose key equals the marker: unclaimed
        self._field = torch.zeros(cap + 1, dtype=torch.int64, device=dev)
        self._value = torch.zeros(cap + 1, dtype=torch.int64, device=dev)
        self._count = torch.zeros(cap + 1, dtype=torch.int64, device=dev)
        self._first = torch.full((cap + 1,), I64_MAX, dtype=torch.int64, device=dev)
        self._last = torch.full((cap + 1,), I64_MIN, dtype=torch.int64, device=dev)
        self._used = torch.zeros(2, dtype=torch.int64, device=dev)

    def _tab(self):
        return (self._key.data_ptr(), self._field.data_ptr(), self._value.data_ptr(), self._count.data_ptr(),
                self._first.data_ptr(), self._last.data_ptr(), self._used.data_ptr(), self.cap)

    def rows(self) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """(field, value, count, first, last) of every entry, int64 each, in no particular order."""
        return self._rows(self.used)

    def _triples(self, who: str, field, value, ord):
        n = field.numel()
        if value.numel() != n or ord.numel() != n:
            raise ValueError("VarTable.%s: field, value and ord differ in length" % who)
        return tuple(t.to(device=self.device, dtype=torch.int64).contiguous() for t in (field, value, ord))

    def fold(self, field: torch.Tensor, value: torch.Tensor, ord: torch.Tensor, skip: Optional[GapTable] = None) -> None:
        """Fold the triples (field[i], value[i], ord[i]) into the table; a triple whose field the
        ``GapTable`` ``skip`` holds (as a signature) is dropped."""
        field, value, ord = self._triples("fold", field, value, ord)
        if skip is not None and skip.device != self.device:
            raise ValueError("VarTable.fold: the skip set lives on %s, the table on %s" % (skip.device, self.device))
        n = field.numel()
        if n == 0:
            return
        self._reserve(n)
        N.var_fold(self._tab(), None if skip is None else skip._tab(), field.data_ptr(), value.data_ptr(), ord.data_ptr(),
                   n, _s(self._key), self._cuda, self.tile)

    def winners(self, field: torch.Tensor, value: torch.Tensor, ord: torch.Tensor) -> torch.Tensor:
        """The indices (int64, no particular order) of the triples whose entry exists and whose
        ``first`` equals their ordinal: after a fold of the same triples, the lines that became a
        value's first line."""
        field, value, ord = self._triples("winners", field, value, ord)
        n = field.numel()
        if n == 0:
            return torch.empty(0, dtype=torch.int64, device=self.device)
        out = torch.empty(n, dtype=torch.int64, device=self.device)
        cnt = torch.zeros(1, dtype=torch.int64, device=self.device)
        N.var_winners(self._tab(), field.data_ptr(), value.data_ptr(), ord.data_ptr(), n, out.data_ptr(), cnt.data_ptr(),
                      _s(self._key), self._cuda)
        return out[:int(cnt.item())]

    def purge(self, fields: torch.Tensor) -> int:
        """Drop every entry whose field is in ``fields`` (int64): the rows, without those, into a
        fresh table of the same capacity -- the path of growth. Returns the entries dropped."""
        fields = fields.to(device=self.device, dtype=torch.int64)
        used = self.used
        if used == 0 or fields.numel() == 0:
            return 0
        rows = self._rows(used)
        keep = ~torch.isin(rows[0], fields)
        kept = int(keep.sum().item())
        if kept == used:
            return 0
        rows = tuple(c[keep].contiguous() for c in rows)
        self._alloc(self.cap)
        self._reinsert(rows, kept)
        self._bound = kept
        return used - kept


# ---------------------------------------------------------------------------------------------
# spans report (csrc/kernels/spans.hip): stamp, signature and sampled keys of every line from one
# visit, the span table (span_table.h)

SK_MAX_LINES = 2048         # lines per block of k_span_keys at most
SPAN_TOK_BYTES = 64         # bytes of a span's token column (KEY_MAX_LEN)
SPAN_LEVELS = 65            # levels of a key: the leading zero bits of its hash, 0..64
KEY_POS_LEN_SHIFT = 10      # a token's place: offset in the line | length << 10 (csrc/kernels/key_core.h)


def span_keys(text, line_start, line_len, min_len: int = 8, shift: int = 0, cap: Optional[int] = None,
              per_block: int = 0, levels: Optional[torch.Tensor] = None):
    """Stamp, template signature and keys of every line from ONE visit: (sig int64[L], ts int64[L],
    line int32[n], key int64[n], tok int32[n], (n, lines with at least one triple)). ``sig`` / ``ts``
    are those of ``line_stamps``; the triples are the keys of ``line_keys`` (every line, no table)
    that lie in the hash sample ``shift`` -- the top ``shift`` bits of ``golden.fmix64(key)`` are
    zero -- each with the place of its token, ``offset in the line | length << 10``. ``levels``
    (int64[65] on the text's device, optional): ``levels[m]`` grows by the lines with a triple whose
    deepest key has ``golden.span_level`` m. One pass over the text (k_span_keys) with the capacity
    protocol of ``line_keys``. ``per_block``: lines per block instead of the size the launch picks
    (tests). GPU: the triples come in no particular order; CPU: in line order, the keys of a line
    in byte order."""
    dev = text.device
    L = line_start.numel()
    if line_start.dtype != torch.int64 or not line_start.is_contiguous():
        raise ValueError("span_keys: line_start must be contiguous int64[L]")
    if line_len.dtype != torch.int32 or line_len.numel() != L or not line_len.is_contiguous():
        raise ValueError("span_keys: line_len must be contiguous int32[L]")
    if text.dtype != torch.uint8 or not text.is_contiguous() or line_start.device != dev or line_len.device != dev:
        raise ValueError("span_keys: text must be contiguous uint8, the line index on its device")
    if not KEY_MIN_LEN <= min_len <= KEY_MAX_LEN:
        raise ValueError("span_keys: min_len must be %d..%d" % (KEY_MIN_LEN, KEY_MAX_LEN))
    if not 0 <= shift <= 64:
        raise ValueError("span_keys: shift must be 0..64")
    if per_block and not 0 < per_block <= SK_MAX_LINES:
        raise ValueError("span_keys: per_block must be 1..%d" % SK_MAX_LINES)
    if levels is not None and (levels.dtype != torch.int64 or levels.numel() != SPAN_LEVELS or levels.device != dev
                               or not levels.is_contiguous()):
        raise ValueError("span_keys: levels must be contiguous int64[%d] on the text's device" % SPAN_LEVELS)
    sig = torch.empty(L, dtype=torch.int64, device=dev)
    ts = torch.empty(L, dtype=torch.int64, device=dev)
    if L == 0:
        return (sig, ts, torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int64, device=dev),
                torch.empty(0, dtype=torch.int32, device=dev), (0, 0))
    # a re-run costs a whole pass over the text, a triple 16 bytes: a line of a service log holds an id or two
    cap = max(1024, 2 * L) if cap is None else max(0, int(cap))
    while True:
        out_line = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
        out_key = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
        out_tok = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
        cnt = torch.zeros(2, dtype=torch.int64, device=dev)
        lvl = None if levels is None else torch.zeros(SPAN_LEVELS, dtype=torch.int64, device=dev)
        N.span_keys(text.data_ptr(), text.numel(), line_start.data_ptr(), line_len.data_ptr(), L, int(min_len), int(shift),
                    sig.data_ptr(), ts.data_ptr(), out_line.data_ptr(), out_key.data_ptr(), out_tok.data_ptr(), cap,
                    cnt.data_ptr(), _p(lvl), _s(text), text.is_cuda, per_block)
        m, lines = cnt.tolist()
        if m <= cap:
            if levels is not None:
                levels += lvl               # (only the run that fits counts)
            return sig, ts, out_line[:m], out_key[:m], out_tok[:m], (m, lines)
        cap = m


class SpanTable(_SlotTable):
    """Device-resident spans per key: per id its pairs (lines), its smallest and largest global
    line number, the smallest and largest effective time of its timed lines, the template
    signatures of its first and last line and the lowered token of its first line, kept across
    ``fold`` calls (the chunks of a stream). GPU: k_span_fold / k_span_ends / k_span_rows /
    k_span_reinsert; CPU: their host twins on the same layout. Capacity and growth: ``_SlotTable``."""

    _max_tile = 2048
    _rows_op, _reinsert_op = "span_rows", "span_reinsert"

    def _alloc(self, cap: int) -> None:
        dev = self.device
        self.cap = cap
        self._key = torch.full((cap + 1,), GT_EMPTY, dtype=torch.int64, device=dev)
        self._key[cap] = 0          # the side slot of the key that equals the marker: unclaimed
        self._count = torch.zeros(cap + 1, dtype=torch.int64, device=dev)
        self._first = torch.full((cap + 1,), I64_MAX, dtype=torch.int64, device=dev)
        self._last = torch.full((cap + 1,), I64_MIN, dtype=torch.int64, device=dev)
        self._tmin = torch.full((cap + 1,), I64_MAX, dtype=torch.int64, device=dev)
        self._tmax = torch.full((cap + 1,), I64_MIN, dtype=torch.int64, device=dev)
        self._opens = torch.zeros(cap + 1, dtype=torch.int64, device=dev)
        self._closes = torch.zeros(cap + 1, dtype=torch.int64, device=dev)
        self._toklen = torch.zeros(cap + 1, dtype=torch.int32, device=dev)
        self._tok = torch.zeros((cap + 1, SPAN_TOK_BYTES), dtype=torch.uint8, device=dev)
        self._used = torch.zeros(2, dtype=torch.int64, device=dev)

    def _tab(self):
        return (self._key.data_ptr(), self._count.data_ptr(), self._first.data_ptr(), self._last.data_ptr(),
                self._tmin.data_ptr(), self._tmax.data_ptr(), self._opens.data_ptr(), self._closes.data_ptr(),
                self._toklen.data_ptr(), self._tok.data_ptr(), self._used.data_ptr(), self.cap)

    def _rows(self, n: int, shift: int = 0):
        """Every column of the occupied slots whose key is in sample ``shift``, in no particular
        order: ``n`` is their number where the caller knows it (``shift == 0``: the occupied
        slots), else an upper bound, and the rows are cut to the number found."""
        dev = self.device
        cols = tuple(torch.empty(n, dtype=torch.int64, device=dev) for _ in range(8)) \
            + (torch.empty(n, dtype=torch.int32, device=dev), torch.empty((n, SPAN_TOK_BYTES), dtype=torch.uint8, device=dev))
        cnt = torch.zeros(1, dtype=torch.int64, device=dev)
        N.span_rows(self._tab(), tuple(c.data_ptr() for c in cols), n, cnt.data_ptr(), _s(self._key), self._cuda, int(shift))
        found = int(cnt.item())
        if found > n or (shift == 0 and found != n):
            raise RuntimeError("SpanTable: %d occupied slots, the counter says %d" % (found, n))
        return cols if found == n else tuple(c[:found].contiguous() for c in cols)

    def rows(self):
        """(key, count, first, last, tmin, tmax, opens, closes: int64[n]; toklen int32[n]; tok
        uint8[n, 64]) of every span, in no particular order. ``tmin > tmax``: no line of the span
        has a time."""
        return self._rows(self.used)

    def fold(self, line: torch.Tensor, key: torch.Tensor, tok: torch.Tensor, sig: torch.Tensor, eff: torch.Tensor,
             text: torch.Tensor, line_start: torch.Tensor, line_base: int) -> None:
        """Fold the triples of ONE ``span_keys`` call -- (line[i], key[i], tok[i]), lines counted
        within the piece -- into the table: fold, then ends. ``sig`` / ``eff`` (int64[L]): the
        signatures and effective times (``TS_NONE``: none) of the piece's lines; ``text`` /
        ``line_start``: the piece itself, from which the tokens are cut; ``line_base``: the global
        number of its line 0. A key whose first line lies in this call gets ``opens`` and its token
        here; ``closes`` is rewritten by every call that raises the key's last line."""
        dev = self.device
        n, L = key.numel(), line_start.numel()
        if line.numel() != n or tok.numel() != n:
            raise ValueError("SpanTable.fold: line, key and tok differ in length")
        if sig.numel() != L or eff.numel() != L:
            raise ValueError("SpanTable.fold: sig and eff must have one entry per line")
        for name, t, dt in (("line", line, torch.int32), ("key", key, torch.int64), ("tok", tok, torch.int32),
                            ("sig", sig, torch.int64), ("eff", eff, torch.int64), ("text", text, torch.uint8),
                            ("line_start", line_start, torch.int64)):
            if t.dtype != dt or t.device != dev or not t.is_contiguous():
                raise ValueError("SpanTable.fold: %s must be contiguous %s on %s" % (name, dt, dev))
        if isinstance(line_base, bool) or not isinstance(line_base, int) or not 0 <= line_base < (1 << 62):
            raise ValueError("SpanTable.fold: line_base must be an integer in [0, 2^62)")
        if n == 0:
            return
        self._reserve(n)
        pairs = (line.data_ptr(), key.data_ptr(), tok.data_ptr(), n, sig.data_ptr(), eff.data_ptr(), L, text.data_ptr(),
                 text.numel(), line_start.data_ptr(), line_base)
        tab, st = self._tab(), _s(self._key)
        N.span_fold(tab, pairs, st, self._cuda)
        N.span_ends(tab, pairs, st, self._cuda)

    def purge(self, shift: int) -> int:
        """Drop every span whose key is outside the hash sample ``shift``: the rows of the sample
        (the filter is k_span_rows' own) into a fresh table of the same capacity -- the path of
        growth. Returns the spans dropped."""
        if not 0 <= shift <= 64:
            raise ValueError("SpanTable.purge: shift must be 0..64")
        used = self.used
        if used == 0 or shift == 0:
            return 0
        rows = self._rows(used, shift)
        kept = rows[0].numel()
        if kept == used:
            return 0
        self._alloc(self.cap)
        self._reinsert(rows, kept)
        self._bound = kept
        return used - kept


# ---------------------------------------------------------------------------------------------
# log timeline (csrc/kernels/timeline.hip): the timestamp of every line, counts per time bucket

TS_NONE = -(1 << 63)       # a line without a stamp / without an effective time (csrc/kernels/ts_core.h)
TL_TILE = 2048              # items (lines, then events) per block of k_tl_hist
TL_LDS_SLOTS = 256          # buckets of its block table at most: more distinct buckets in a tile go to HBM directly


def line_timestamps(text, line_start, line_len) -> torch.Tensor:
    """Epoch milliseconds (UTC) of the stamp at the head of every line (int64[L], ``TS_NONE``
    where a line has none; ``golden.line_timestamp``): k_ts_parse or its host twin."""
    L = line_start.numel()
    if line_start.dtype != torch.int64 or not line_start.is_contiguous():
        raise ValueError("line_timestamps: line_start must be contiguous int64[L]")
    if line_len.dtype != torch.int32 or line_len.numel() != L or not line_len.is_contiguous():
        raise ValueError("line_timestamps: line_len must be contiguous int32[L]")
    if text.dtype != torch.uint8 or not text.is_contiguous() or line_start.device != text.device \
            or line_len.device != text.device:
        raise ValueError("line_timestamps: text must be contiguous uint8, the line index on its device")
    out = torch.empty(L, dtype=torch.int64, device=text.device)
    if L:
        N.ts_parse(text.data_ptr(), text.numel(), line_start.data_ptr(), line_len.data_ptr(), L, out.data_ptr(),
                   _s(text), text.is_cuda)
    return out


LS_MAX_LINES = 2048         # lines per block of k_line_stamps at most (csrc/kernels/trends.hip)


def line_stamps(text, line_start, line_len, per_block: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """(sig int64[L], ts int64[L]): template signature (``golden.line_signature``) and stamp
    (``golden.line_timestamp``, ``TS_NONE`` where the line has none) of every line from ONE visit
    of the line -- what ``line_signatures`` and ``line_timestamps`` give in two launches.
    k_line_stamps or its host twin. ``per_block``: lines per block instead of the size the launch
    picks (tests)."""
    L = line_start.numel()
    if line_start.dtype != torch.int64 or not line_start.is_contiguous():
        raise ValueError("line_stamps: line_start must be contiguous int64[L]")
    if line_len.dtype != torch.int32 or line_len.numel() != L or not line_len.is_contiguous():
        raise ValueError("line_stamps: line_len must be contiguous int32[L]")
    if text.dtype != torch.uint8 or not text.is_contiguous() or line_start.device != text.device \
            or line_len.device != text.device:
        raise ValueError("line_stamps: text must be contiguous uint8, the line index on its device")
    if per_block and not 0 < per_block <= LS_MAX_LINES:
        raise ValueError("line_stamps: per_block must be 1..%d" % LS_MAX_LINES)
    sig = torch.empty(L, dtype=torch.int64, device=text.device)
    ts = torch.empty(L, dtype=torch.int64, device=text.device)
    if L:
        N.line_stamps(text.data_ptr(), text.numel(), line_start.data_ptr(), line_len.data_ptr(), L, sig.data_ptr(),
                      ts.data_ptr(), _s(text), text.is_cuda, per_block)
    return sig, ts


def timeline_fill(ts: torch.Tensor, carry_last: int = TS_NONE,
                  carry_top: int = TS_NONE) -> Tuple[torch.Tensor, torch.Tensor]:
    """Effective times and the out-of-order count of the stamps ``ts`` (int64[L], line order):
    (eff int64[L], count int64[1] on the device). ``eff[i]`` is the stamp of the nearest stamped
    line at or before i -- the nearest, not the largest -- else ``carry_last``; a stamped line
    counts as out of order when its stamp is below the largest stamp before it (``carry_top``
    included). The carries continue the scans across the chunks of a stream. k_tl_tiles /
    k_tl_prefix / k_tl_fill or their host twin."""
    if ts.dtype != torch.int64 or not ts.is_contiguous():
        raise ValueError("timeline_fill: ts must be contiguous int64[L]")
    L = ts.numel()
    eff = torch.empty_like(ts)
    ooo = torch.zeros(1, dtype=torch.int64, device=ts.device)
    if L:
        tmp = torch.empty(N.tl_fill_tmp_words(L), dtype=torch.int64, device=ts.device) if ts.is_cuda else None
        N.tl_fill(ts.data_ptr(), L, int(carry_last), int(carry_top), eff.data_ptr(), ooo.data_ptr(), _p(tmp), _s(ts),
                  ts.is_cuda)
    return eff, ooo


PS_TILE = 2048              # lines per block of k_ps_tiles / k_ps_emit (csrc/kernels/pauses.hip)
PS_BUCKETS = 64             # interval histogram: bucket = bit length of the step
PS_STAMPED, PS_BACKWARD, PS_PAUSED_MS, PS_MIN_TS, PS_MAX_TS = range(5)     # columns of its statistics
PS_MAX_ABS_TS = 1 << 61     # stamps lie within +-2^61, so that no step overflows


def pause_stats(device) -> torch.Tensor:
    """Statistics of no line at all: what ``pause_scan`` adds a run to."""
    return torch.tensor([0, 0, 0, I64_MAX, -I64_MAX - 1], dtype=torch.int64, device=device)


def pause_scan(ts: torch.Tensor, sig: torch.Tensor, min_ms: int, line_base: int = 0, carry=None,
               stats: Optional[torch.Tensor] = None, hist: Optional[torch.Tensor] = None):
    """The steps between the stamped lines of a run (``ts`` / ``sig``: int64[L], what
    ``line_stamps`` gives; line i has the global number ``line_base + i``). ``carry``: None, or
    (stamp, global line, signature) of the last stamped line of the earlier runs. Returns

    * rows: (to_line, from_line, ms, from_sig, to_sig), int64[m] each: the steps ``>= min_ms``,
      in line order;
    * stats int64[5] on the device: stamped lines, backward steps, the sum of the rows' ms,
      smallest and largest stamp (``pause_stats``: none). With ``stats`` given the run is added
      to that tensor, which is returned;
    * hist int64[64]: the steps >= 0 by bit length (``hist`` given: added to it);
    * the new carry (None: still no stamped line).

    k_ps_tiles / k_ps_prefix / k_ps_emit or their host twin; the row count and the carry are
    the one read in between. Nothing is launched at L = 0."""
    dev = ts.device
    if ts.dtype != torch.int64 or not ts.is_contiguous() or ts.dim() != 1:
        raise ValueError("pause_scan: ts must be contiguous int64[L]")
    L = ts.numel()
    if sig.dtype != torch.int64 or sig.numel() != L or not sig.is_contiguous() or sig.device != dev:
        raise ValueError("pause_scan: sig must be contiguous int64[L] on the device of ts")
    if isinstance(min_ms, bool) or not isinstance(min_ms, int) or not 1 <= min_ms <= I64_MAX:
        raise ValueError("pause_scan: min_ms must be an integer >= 1")
    if isinstance(line_base, bool) or not isinstance(line_base, int) or not 0 <= line_base <= I64_MAX - L:
        raise ValueError("pause_scan: line_base out of range")
    if carry is not None:
        c_ts, c_line, c_sig = (int(x) for x in carry)
        if not -PS_MAX_ABS_TS <= c_ts <= PS_MAX_ABS_TS or not 0 <= c_line < line_base:
            raise ValueError("pause_scan: the carry is (stamp within +-2^61, line before line_base, signature)")
    else:
        c_ts, c_line, c_sig = TS_NONE, -1, 0
    for name, t, n in (("stats", stats, 5), ("hist", hist, PS_BUCKETS)):
        if t is not None and (t.dtype != torch.int64 or t.numel() != n or not t.is_contiguous() or t.device != dev):
            raise ValueError("pause_scan: %s must be contiguous int64[%d] on the device of ts" % (name, n))
    stats = pause_stats(dev) if stats is None else stats
    hist = torch.zeros(PS_BUCKETS, dtype=torch.int64, device=dev) if hist is None else hist
    if L == 0:
        return tuple(torch.empty(0, dtype=torch.int64, device=dev) for _ in range(5)), stats, hist, carry
    tmp = torch.empty(N.pause_tmp_words(L), dtype=torch.int64, device=dev) if ts.is_cuda else None
    head = torch.empty(4, dtype=torch.int64, device=dev)
    none = (0, 0, 0, 0, 0)
    args = (ts.data_ptr(), sig.data_ptr(), L, line_base, min_ms, c_ts, c_line, c_sig, _p(tmp), head.data_ptr())
    N.pause_scan(False, *args, none, 0, 0, 0, _s(ts), ts.is_cuda)
    m, n_ts, n_line, n_sig = head.tolist()
    rows = tuple(torch.empty(m, dtype=torch.int64, device=dev) for _ in range(5))
    N.pause_scan(True, *args, tuple(r.data_ptr() for r in rows), m, stats.data_ptr(), hist.data_ptr(), _s(ts),
                 ts.is_cuda)
    return rows, stats, hist, (None if n_ts == TS_NONE else (n_ts, n_line, n_sig))


CD_TILE = 2048              # lines per block of k_cd_tile (csrc/kernels/cadence.hip)
CDL_ROWS = 256              # rows per block of k_cdl_tiles / k_cdl_emit
# columns of a cadence state (csrc/kernels/lp_api.h)
(CD_SIG, CD_LINES, CD_BEATS, CD_BACKWARD, CD_SUM, CD_MIN, CD_MAX, CD_MAX_FROM, CD_MAX_TO, CD_FIRST_LINE, CD_LAST_LINE,
 CD_LAST_TS, CD_FIRST_TS, CD_MAX_TO_TS) = range(14)
CD_COLS = 14


def beat_state(device) -> torch.Tensor:
    """The cadence state of no line at all."""
    return torch.empty((CD_COLS, 0), dtype=torch.int64, device=device)


def beat_scan(ts: torch.Tensor, sig: torch.Tensor, line_base: int = 0, state: Optional[torch.Tensor] = None,
              cap: Optional[int] = None):
    """Per stamped line the *beat* since the previous stamped line of the same template, and the
    templates' running rows (``ts`` / ``sig``: int64[L], what ``line_stamps`` gives; line i has the
    global number ``line_base + i``). ``state``: None, or what an earlier call returned for the
    lines before ``line_base``. Returns

    * beat int64[L]: the line's stamp minus the stamp of the previous stamped line of its
      signature -- in this run or, through ``state``, before it; ``TS_NONE`` for an unstamped line
      and for the first stamped line of a signature;
    * bkt int64[L]: the bit length of a beat >= 0 (``golden.pause_bucket``), else ``TS_NONE`` --
      the ``eff`` column of ``CellTable.fold(sig, bkt, line_base, 1)``;
    * the new state int64[CD_COLS, T]: one row per signature seen so far, sorted by signature (as
      a signed number); columns ``CD_SIG .. CD_MAX_TO_TS``. The state after runs A then B is the
      state of the one run A + B, bit for bit.

    k_cd_tile writes one row per (tile of 2,048 lines, signature) with the capacity protocol of
    ``novel_lines`` (``cap``: rows of the first try); state rows and tile rows are sorted by first
    line, then stably by signature, with torch; k_cdl_tiles / k_cdl_prefix / k_cdl_emit join the
    rows of a signature in that order and write the beats across tile and run borders. CPU: the
    host twins. The row counts are the two small reads."""
    dev = ts.device
    if ts.dtype != torch.int64 or not ts.is_contiguous() or ts.dim() != 1:
        raise ValueError("beat_scan: ts must be contiguous int64[L]")
    L = ts.numel()
    if sig.dtype != torch.int64 or sig.dim() != 1 or sig.numel() != L or not sig.is_contiguous() or sig.device != dev:
        raise ValueError("beat_scan: sig must be contiguous int64[L] on the device of ts")
    if isinstance(line_base, bool) or not isinstance(line_base, int) or not 0 <= line_base <= I64_MAX - L:
        raise ValueError("beat_scan: line_base out of range")
    if state is None:
        state = beat_state(dev)
    elif (not isinstance(state, torch.Tensor) or state.dtype != torch.int64 or state.dim() != 2
          or state.shape[0] != CD_COLS or not state.is_contiguous() or state.device != dev):
        raise ValueError("beat_scan: state must be contiguous int64[%d, T] on the device of ts" % CD_COLS)
    if state.shape[1] and line_base == 0:
        raise ValueError("beat_scan: a state speaks of lines before line_base")
    if cap is not None and (isinstance(cap, bool) or not isinstance(cap, int) or cap < 0):
        raise ValueError("beat_scan: cap must be None or an integer >= 0")
    beat = torch.empty(L, dtype=torch.int64, device=dev)
    bkt = torch.empty(L, dtype=torch.int64, device=dev)
    if L == 0:
        return beat, bkt, state
    rows = beat_tile_rows(ts, sig, line_base, beat, bkt, cap)
    rows = beat_sort_rows(torch.cat([state, rows], dim=1))
    return beat, bkt, beat_link_rows(rows, line_base, beat, bkt)


def beat_tile_rows(ts, sig, line_base: int, beat, bkt, cap: Optional[int] = None) -> torch.Tensor:
    """First step of ``beat_scan`` (its checks made): k_cd_tile. Writes ``beat`` / ``bkt`` inside
    the tiles and returns the tile rows int64[CD_COLS, n]; the read of n is the capacity protocol."""
    L, dev = ts.numel(), ts.device
    cap = min(L, max(1024, L // 4)) if cap is None else cap
    while True:
        rows = torch.empty((CD_COLS, max(cap, 1)), dtype=torch.int64, device=dev)
        cnt = torch.zeros(1, dtype=torch.int64, device=dev)
        N.cadence_tile(ts.data_ptr(), sig.data_ptr(), L, line_base, beat.data_ptr(), bkt.data_ptr(), rows.data_ptr(),
                       cap, cnt.data_ptr(), _s(ts), ts.is_cuda)
        n = int(cnt.item())
        if n <= cap:
            return rows[:, :n]
        cap = n


def beat_sort_rows(rows: torch.Tensor) -> torch.Tensor:
    """Second step: the rows by (signature, first line). A state row lies before line_base and
    leads its group. The sorts wipe the order the block atomics gave the tile rows."""
    o = torch.sort(rows[CD_FIRST_LINE], stable=True)[1]
    o = o[torch.sort(rows[CD_SIG][o], stable=True)[1]]
    return rows[:, o].contiguous()


def beat_link_rows(rows: torch.Tensor, line_base: int, beat, bkt) -> torch.Tensor:
    """Third step: k_cdl_tiles / k_cdl_prefix / k_cdl_emit over the sorted rows. Writes the beats
    across tile and run borders and returns the new state; the read of its row count."""
    dev, R, L = rows.device, rows.shape[1], beat.numel()
    out = torch.empty((CD_COLS, max(R, 1)), dtype=torch.int64, device=dev)
    head = torch.empty(1, dtype=torch.int64, device=dev)
    tmp = torch.empty(N.cadence_link_tmp_words(R), dtype=torch.int64, device=dev) if rows.is_cuda else None
    N.cadence_link(rows.data_ptr(), R, out.data_ptr(), max(R, 1), head.data_ptr(), _p(tmp), line_base, L,
                   beat.data_ptr(), bkt.data_ptr(), _s(rows), rows.is_cuda)
    return out[:, :int(head.item())].contiguous()


def timeline_hist(eff: torch.Tensor, feat: torch.Tensor, ev_line: torch.Tensor, ev_pat: torch.Tensor,
                  sev_index: torch.Tensor, t0: int, W: int, nb: int, S: int) -> torch.Tensor:
    """int64[nb, 3 + S]: per bucket ``[t0 + b * W, t0 + (b + 1) * W)`` the lines whose effective
    time ``eff`` (int64[L], ``TS_NONE``: undated) falls into it, those of them that are error
    lines (``feat``: uint8[L] context features), the events on them (``ev_line`` / ``ev_pat``:
    int32[E]) and these per severity (``sev_index``: int32[P]). Undated lines and events, and
    times outside the nb buckets, are counted nowhere. k_tl_hist or its host twin."""
    dev = eff.device
    L, E = eff.numel(), ev_line.numel()
    if eff.dtype != torch.int64 or not eff.is_contiguous():
        raise ValueError("timeline_hist: eff must be contiguous int64[L]")
    if feat.dtype != torch.uint8 or feat.numel() < L or not feat.is_contiguous():
        raise ValueError("timeline_hist: feat must be contiguous uint8[L]")
    if ev_pat.numel() != E:
        raise ValueError("timeline_hist: ev_line and ev_pat differ in length")
    if W < 1 or not 1 <= nb < (1 << 31) or S < 0:
        raise ValueError("timeline_hist: need W >= 1, 1 <= nb < 2^31, S >= 0")
    ev_line = ev_line.to(device=dev, dtype=torch.int32).contiguous()
    ev_pat = ev_pat.to(device=dev, dtype=torch.int32).contiguous()
    sev_index = sev_index.to(device=dev, dtype=torch.int32).contiguous()
    hist = torch.zeros((nb, 3 + S), dtype=torch.int64, device=dev)
    if L + E:
        N.tl_hist(eff.data_ptr(), feat.data_ptr(), L, ev_line.data_ptr(), ev_pat.data_ptr(), E, sev_index.data_ptr(),
                  sev_index.numel(), S, int(t0), int(W), int(nb), hist.data_ptr(), _s(eff), eff.is_cuda)
    return hist


# ---------------------------------------------------------------------------------------------
# trace report (csrc/kernels/traces.hip): stack traces as runs of frame / cause lines

TR_OTHER, TR_FRAME, TR_MORE, TR_CAUSE = 0, 1, 2, 3      # line classes (csrc/kernels/trace_core.h)
TR_TILE = 1024              # lines per block of k_tr_tiles / k_tr_emit
TR_COLS = 8                 # columns of a trace row:
TR_START, TR_SIG, TR_LINES, TR_FRAMES, TR_CAUSES, TR_FLAGS, TR_FF, TR_LC = range(8)
TR_ROW_EVENT, TR_ROW_HEADLESS = 1, 2                    # its flag bits
TR_NO_CAUSE = -(1 << 63)    # last CAUSE line of a trace without one
TR_CARRY_WORDS = 13
# the words of a carry: an open run (pow and val as int64 bit patterns; line numbers count from
# the next piece's first line), an event on the previous line, there is a previous line
(TRC_OPEN, TRC_POW, TRC_VAL, TRC_FRAMES, TRC_CAUSES, TRC_LINES, TRC_EVENT, TRC_HEADLESS, TRC_START, TRC_FF, TRC_LC,
 TRC_PREV_EVENT, TRC_HAS_PREV) = range(13)
TR_CARRY_START = (0, 1, 0, 0, 0, 0, 0, 0, 0, (1 << 63) - 1, -(1 << 63), 0, 0)     # the document begins here


def trace_classes(text, line_start, line_len) -> Tuple[torch.Tensor, torch.Tensor]:
    """(class uint8[L], element int64[L]) of every line: ``golden.trace_class`` and the bit pattern
    of ``golden.trace_element`` (0 where a line contributes nothing). k_tr_class or its host twin;
    the template signature is computed on FRAME lines only."""
    L = line_start.numel()
    dev = text.device
    if line_start.dtype != torch.int64 or not line_start.is_contiguous() or line_start.device != dev:
        raise ValueError("trace_classes: line_start must be contiguous int64[L] on the text's device")
    if line_len.dtype != torch.int32 or line_len.numel() != L or not line_len.is_contiguous() or line_len.device != dev:
        raise ValueError("trace_classes: line_len must be contiguous int32[L] on the text's device")
    if text.dtype != torch.uint8 or not text.is_contiguous():
        raise ValueError("trace_classes: text must be contiguous uint8")
    cls = torch.empty(L, dtype=torch.uint8, device=dev)
    elem = torch.empty(L, dtype=torch.int64, device=dev)
    if L:
        N.trace_class(text.data_ptr(), text.numel(), line_start.data_ptr(), line_len.data_ptr(), L, cls.data_ptr(),
                      elem.data_ptr(), _s(text), text.is_cuda)
    return cls, elem


def trace_runs(text, line_start, line_len, ev_mask: Optional[torch.Tensor] = None, carry=TR_CARRY_START,
               last: bool = True, cap: Optional[int] = None):
    """The stack traces that end in the lines (line_start, line_len) of ``text``, one piece of a
    document: (columns int64[TR_COLS, n], (n,), carry_out). A run is a maximal sequence of
    consecutive non-OTHER lines, a trace a run with a FRAME. Columns: start line, signature
    (``golden.trace_signature``'s bit pattern), run lines, frames, causes, flags (bit0: an event
    of ``ev_mask`` -- uint8[L]; None: no events -- lies on the head or a run line, bit1: headless),
    first FRAME line, last CAUSE line (``TR_NO_CAUSE`` without one). Line numbers count from the
    piece's first line; those of a run that came in with ``carry`` are negative. ``carry``: what
    the previous piece's call returned (``TR_CARRY_START`` for the first piece); ``last``: no
    piece follows, a run that reaches the last line ends there -- otherwise it goes out in
    ``carry_out`` and no row is written for it yet. k_tr_class, then the segmented scan k_tr_tiles
    / k_tr_prefix / k_tr_emit, or their host twins, with the capacity protocol of ``novel_lines``.
    GPU: the rows come in no particular order; CPU: in line order."""
    dev = text.device
    L = line_start.numel()
    carry = tuple(int(c) for c in carry)
    if len(carry) != TR_CARRY_WORDS:
        raise ValueError("trace_runs: the carry has %d words" % TR_CARRY_WORDS)
    if ev_mask is not None and (ev_mask.dtype != torch.uint8 or ev_mask.numel() < L or not ev_mask.is_contiguous()
                                or ev_mask.device != dev):
        raise ValueError("trace_runs: ev_mask must be contiguous uint8[L] on the text's device")
    if L == 0:
        # no line: the carry passes through, or (last) the run that came in ends here
        cols = torch.empty((TR_COLS, 0), dtype=torch.int64, device=dev)
        if not last:
            return cols, (0,), carry
        out = (0, 1, 0, 0, 0, 0, 0, 0, 0) + TR_CARRY_START[9:11] + (carry[TRC_PREV_EVENT], carry[TRC_HAS_PREV])
        if carry[TRC_OPEN] and carry[TRC_FRAMES] > 0:
            cols = torch.tensor(_carry_row(carry), dtype=torch.int64, device=dev).reshape(TR_COLS, 1)
        return cols, (int(cols.shape[1]),), out
    cls, elem = trace_classes(text, line_start, line_len)
    cap = max(64, L // 64) if cap is None else max(1, int(cap))
    tmp = torch.empty(N.trace_runs_tmp_bytes(L) // 8, dtype=torch.int64, device=dev) if text.is_cuda else None
    while True:
        out = torch.empty((TR_COLS, cap), dtype=torch.int64, device=dev)
        state = torch.zeros(1 + TR_CARRY_WORDS, dtype=torch.int64, device=dev)      # the count, then the carry out
        N.trace_runs(cls.data_ptr(), elem.data_ptr(), _p(ev_mask), L, carry, bool(last), out.data_ptr(), cap,
                     state.data_ptr(), state.data_ptr() + 8, _p(tmp), _s(text), text.is_cuda)
        n, *carry_out = state.tolist()
        if n <= cap:
            return out[:, :n], (n,), tuple(carry_out)
        cap = n


def _carry_row(carry) -> list:
    """The trace row of an open run that ends where it stands (csrc/kernels/trace_core.h tr_row)."""
    from ..golden import fmix64
    sig = fmix64((carry[TRC_VAL] ^ (carry[TRC_FRAMES] + carry[TRC_CAUSES])) & ((1 << 64) - 1))
    flags = (TR_ROW_EVENT if carry[TRC_EVENT] else 0) | (TR_ROW_HEADLESS if carry[TRC_HEADLESS] else 0)
    return [carry[TRC_START], sig - (1 << 64) if sig >> 63 else sig, carry[TRC_LINES], carry[TRC_FRAMES],
            carry[TRC_CAUSES], flags, carry[TRC_FF], carry[TRC_LC]]
