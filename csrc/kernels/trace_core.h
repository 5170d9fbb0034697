// Stack traces of the trace report (traces.hip): the class of a line (frame, "... n more", cause,
// anything else), what a run line contributes to its trace's signature, and the aggregate of a run
// of consecutive non-OTHER lines with its associative combine (log_parser_amd/golden.py traces is
// the specification). One source for the gfx950 kernels and their host twin, as in gaps_core.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gap_table.h"
#include "gaps_core.h"
#include "lp_core.h"

namespace lp {

constexpr uint8_t TR_OTHER = 0, TR_FRAME = 1, TR_MORE = 2, TR_CAUSE = 3;
constexpr int TR_LEAD_MAX = 64;      // blanks in front of "at" / "..." / "Caused by:" at most
constexpr int TR_GAP_MAX = 8;        // blanks between the colon and the cause token that are skipped
constexpr int TR_TOKEN_MAX = 256;    // bytes of the cause token that count
// the longest prefix that decides: 65 blanks, or 64 + "Suppressed:" + 8 + 256 and the byte after
constexpr int TR_PREFIX_MAX = TR_LEAD_MAX + 11 + TR_GAP_MAX + TR_TOKEN_MAX + 1;
constexpr uint64_t TR_M = 0x9E3779B97F4A7C15ull;

// ---- the class of a line: a byte-at-a-time automaton over a bounded prefix
struct TrClassState {
  uint32_t ph = 0;     // 0 lead-in, 1 "at", 2 "...", 3 "Caused by:", 4 "Suppressed:", 5 gap, 6 token, 7 decided
  uint32_t cnt = 0;    // blanks / keyword bytes / gap blanks / token bytes so far
  uint32_t cls = TR_OTHER;
  uint64_t h = SIG_FNV_OFFSET;   // FNV-1a-64 of the cause token
};

// byte k of "Caused by:" (which = 0) or "Suppressed:" (which = 1), packed little-endian
LP_HD uint32_t tr_kw(int which, uint32_t k) {
  const uint64_t lo = which ? 0x7373657270707553ull : 0x6220646573756143ull;   // "Suppress" / "Caused b"
  const uint64_t hi = which ? 0x00000000003a6465ull : 0x0000000000003a79ull;   // "ed:" / "y:"
  return (uint32_t)(((k < 8 ? lo : hi) >> (8 * (k & 7))) & 0xFFu);
}

LP_HD void tr_class_step(TrClassState& S, uint32_t c) {
  const bool ws = c == ' ' || c == '\t';
  switch (S.ph) {
    case 0:
      if (ws) {
        if (++S.cnt > (uint32_t)TR_LEAD_MAX) S.ph = 7;
      } else {
        const bool led = S.cnt >= 1;
        S.ph = (c == 'a' && led) ? 1u : (c == '.' && led) ? 2u : c == 'C' ? 3u : c == 'S' ? 4u : 7u;
        S.cnt = 1;
      }
      break;
    case 1:
      if (S.cnt == 1 && c == 't') {
        S.cnt = 2;
      } else {
        if (S.cnt == 2 && ws) S.cls = TR_FRAME;
        S.ph = 7;
      }
      break;
    case 2:
      if (c != '.') {
        S.ph = 7;
      } else if (++S.cnt == 3) {
        S.cls = TR_MORE;
        S.ph = 7;
      }
      break;
    case 3:
    case 4: {
      const uint32_t len = S.ph == 3 ? 10u : 11u;
      if (c != tr_kw(S.ph == 4, S.cnt)) {
        S.ph = 7;
      } else if (++S.cnt == len) {
        S.cls = TR_CAUSE;     // from here on the line is a cause, wherever it ends
        S.ph = 5;
        S.cnt = 0;
      }
      break;
    }
    case 5:
      if (ws && S.cnt < (uint32_t)TR_GAP_MAX) {
        ++S.cnt;
        break;
      }
      S.ph = 6;
      S.cnt = 0;
      [[fallthrough]];
    case 6:
      if (ws || c == ':') {
        S.ph = 7;
      } else {
        S.h = sig_fold(S.h, c);
        if (++S.cnt == (uint32_t)TR_TOKEN_MAX) S.ph = 7;
      }
      break;
    default:
      break;
  }
}

// class of the line text[start, start + n), and the hash of its cause token in *token (CAUSE
// only). Device: aligned 16-byte loads with the lead-in of the first block masked, as in
// line_sig_at, and no block beyond the one that decides; never a byte before `text`, at / after
// text + tbytes or past the line's own length.
LP_HD uint8_t trace_class_at(const uint8_t* __restrict__ text, int64_t tbytes, int64_t start, int n, uint64_t* token) {
  if (start < 0) start = 0;
  if (start > tbytes) start = tbytes;
  if (n > TR_PREFIX_MAX) n = TR_PREFIX_MAX;
  if ((int64_t)n > tbytes - start) n = (int)(tbytes - start);
  TrClassState S;
#if defined(__HIP_DEVICE_COMPILE__)
  if (n > 0) {
    const int sh = (int)(start & 15);
    int64_t off = start - sh;
    for (int t0 = -sh; t0 < n && S.ph != 7; t0 += 16, off += 16) {
      const uint4 cur = sig_ld16(text, tbytes, off);
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int t = t0 + j;
        const uint32_t w = (j < 4) ? cur.x : (j < 8) ? cur.y : (j < 12) ? cur.z : cur.w;
        if ((t >= 0) & (t < n)) tr_class_step(S, (w >> (8 * (j & 3))) & 0xFFu);
      }
    }
  }
#else
  for (int t = 0; t < n && S.ph != 7; ++t) tr_class_step(S, text[start + t]);
#endif
  *token = S.h;
  return (uint8_t)S.cls;
}

// what a run line contributes to the signature of its trace (0 and no weight for MORE)
LP_HD uint64_t trace_element(const uint8_t* __restrict__ text, int64_t tbytes, int64_t start, int n, uint8_t* cls) {
  uint64_t token;
  const uint8_t c = trace_class_at(text, tbytes, start, n, &token);
  *cls = c;
  if (c == TR_FRAME) return gt_hash((int64_t)line_sig_at(text, tbytes, start, n));
  if (c == TR_CAUSE) return gt_hash((int64_t)~token);
  return 0;
}

// ---- the aggregate of consecutive lines inside one piece: what the scan carries. Line numbers
// count from the piece's first line and the counters are 32 bits wide (a piece has fewer than 2^31
// lines); a run that came in from earlier pieces is joined in 64 bits where it ends (TrOpen).
constexpr int32_t TR_NO_FF = INT32_MAX;   // no FRAME among the lines
constexpr int32_t TR_NO_LC = -1;          // no CAUSE among the lines
constexpr uint32_t TR_CLOSED = 1;         // an OTHER line is among them: the aggregate is of the lines after the last one
constexpr uint32_t TR_EVENT = 2;          // an event lies on one of the run lines

struct TrAgg {
  uint64_t pow, val;                 // the hash pair: M^k and sum(e_i * M^(k - i))
  uint32_t frames, causes, lines;    // k = frames + causes; the run begins at (last line + 1 - lines)
  int32_t ff, lc;                    // first FRAME line, last CAUSE line
  uint32_t flags;
};

LP_HD TrAgg tr_identity() { return TrAgg{1ull, 0ull, 0u, 0u, 0u, TR_NO_FF, TR_NO_LC, 0u}; }

// the aggregate of line i alone
LP_HD TrAgg tr_line(uint8_t cls, uint64_t e, bool event, int32_t i) {
  TrAgg a = tr_identity();
  if (cls == TR_OTHER) {
    a.flags = TR_CLOSED;
    return a;
  }
  const bool hashed = cls == TR_FRAME || cls == TR_CAUSE;
  a.pow = hashed ? TR_M : 1ull;
  a.val = hashed ? e : 0ull;
  a.frames = cls == TR_FRAME;
  a.causes = cls == TR_CAUSE;
  a.lines = 1;
  a.ff = cls == TR_FRAME ? i : TR_NO_FF;
  a.lc = cls == TR_CAUSE ? i : TR_NO_LC;
  a.flags = event ? TR_EVENT : 0u;
  return a;
}

// a's lines, then b's: associative (the hash pair is the composition of x -> x * pow + val)
LP_HD TrAgg tr_combine(const TrAgg& a, const TrAgg& b) {
  if (b.flags & TR_CLOSED) return b;
  TrAgg r;
  r.pow = a.pow * b.pow;
  r.val = a.val * b.pow + b.val;
  r.frames = a.frames + b.frames;
  r.causes = a.causes + b.causes;
  r.lines = a.lines + b.lines;
  r.ff = a.ff < b.ff ? a.ff : b.ff;
  r.lc = a.lc > b.lc ? a.lc : b.lc;
  r.flags = a.flags | b.flags;
  return r;
}

LP_HD int64_t trace_sig_finish(uint64_t val, uint64_t k) { return (int64_t)gt_hash((int64_t)(val ^ k)); }

// ---- a run across pieces: the carry of a stream, int64 words (TR_CARRY_WORDS of them). Line
// numbers count from the first line of the NEXT piece, so they are negative.
constexpr int64_t TR_NONE_FF = INT64_MAX, TR_NONE_LC = INT64_MIN;
constexpr int TR_CARRY_WORDS = 13;
struct TrCarry {
  int64_t open;                      // 1: the previous piece ended inside a run, described below
  uint64_t pow, val;
  int64_t frames, causes, lines;
  int64_t event;                     // an event on the head or on a run line so far
  int64_t headless;
  int64_t start, ff, lc;
  int64_t prev_event;                // an event lies on the previous piece's last line
  int64_t has_prev;                  // there is a previous line (0: this piece begins the document)
};

// a trace row, as the columns of the output (TR_COLS of them)
constexpr int TR_COLS = 8;
constexpr int64_t TR_ROW_EVENT = 1, TR_ROW_HEADLESS = 2;
struct TrRow {
  int64_t start, sig, lines, frames, causes, flags, ff, lc;
};

// The run that ends with line i (inclusive aggregate A of the piece's lines [0, i]) as a carry
// whose line numbers count from `origin`: joined with the run that came in when it reaches back to
// the piece's first line, and with the event on its head.
LP_HD TrCarry tr_close(const TrAgg& A, int64_t i, const TrCarry& in, const uint8_t* __restrict__ evm, int64_t origin) {
  TrCarry r;
  r.open = 1;
  r.prev_event = 0;
  r.has_prev = 1;
  const int64_t ff = A.ff == TR_NO_FF ? TR_NONE_FF : (int64_t)A.ff - origin;
  const int64_t lc = A.lc == TR_NO_LC ? TR_NONE_LC : (int64_t)A.lc - origin;
  const bool ev = (A.flags & TR_EVENT) != 0;
  if ((A.flags & TR_CLOSED) || !in.open) {
    const int64_t start = i + 1 - (int64_t)A.lines;        // > 0 when closed: the line before is OTHER
    r.pow = A.pow;
    r.val = A.val;
    r.frames = A.frames;
    r.causes = A.causes;
    r.lines = A.lines;
    r.headless = (start <= 0 && !in.has_prev) ? 1 : 0;
    const bool head_ev = start > 0 ? (evm && evm[start - 1]) : (in.has_prev && in.prev_event);
    r.event = (ev || head_ev) ? 1 : 0;
    r.start = start - origin;
    r.ff = ff;
    r.lc = lc;
  } else {
    r.pow = in.pow * A.pow;
    r.val = in.val * A.pow + A.val;
    r.frames = in.frames + A.frames;
    r.causes = in.causes + A.causes;
    r.lines = in.lines + A.lines;
    r.headless = in.headless;
    r.event = (in.event || ev) ? 1 : 0;
    r.start = in.start - origin;
    r.ff = in.ff != TR_NONE_FF ? in.ff - origin : ff;
    r.lc = lc != TR_NONE_LC ? lc : (in.lc != TR_NONE_LC ? in.lc - origin : TR_NONE_LC);
  }
  return r;
}

LP_HD TrRow tr_row(const TrCarry& c) {
  return TrRow{c.start, trace_sig_finish(c.val, (uint64_t)(c.frames + c.causes)), c.lines, c.frames, c.causes,
               (c.event ? TR_ROW_EVENT : 0) | (c.headless ? TR_ROW_HEADLESS : 0), c.ff, c.lc};
}

// nothing open after a piece whose last line is OTHER, or after the last piece
LP_HD TrCarry tr_no_carry(bool prev_event) {
  TrCarry r{};
  r.pow = 1;
  r.ff = TR_NONE_FF;
  r.lc = TR_NONE_LC;
  r.prev_event = prev_event ? 1 : 0;
  r.has_prev = 1;
  return r;
}

}  // namespace lp
