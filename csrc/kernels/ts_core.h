// Line timestamps of the timeline report (timeline.hip): the stamp at the head of a line as epoch
// milliseconds, UTC (log_parser_amd/golden.py line_timestamp is the specification). The stamp is
// the leftmost match, starting before byte TS_MAX_START, of
//
//   (?<![0-9A-Za-z])YYYY[-/]MM[-/]DD[T ]hh:mm:ss  (?:[.,]d{1,9})?  (Z|[+-]hh:?mm)?
//
// One source for the gfx950 kernel and its host twin, as in gaps_core.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gaps_core.h"
#include "lp_core.h"

namespace lp {

constexpr int64_t TS_NONE = INT64_MIN;   // the line has no stamp
constexpr int TS_MAX_START = 32;         // a stamp starts at a byte offset below this
constexpr int TS_CORE = 19;              // bytes of the mandatory part, YYYY-MM-DDThh:mm:ss
constexpr int TS_MAX_BYTES = TS_MAX_START - 1 + TS_CORE + 10 + 6;   // 67: no byte behind it is read

// days since 1970-01-01 of a Gregorian date (era / day-of-era form, integers only)
LP_HD int64_t ts_days_from_civil(int y, int m, int d) {
  y -= m <= 2;
  const int era = (y >= 0 ? y : y - 399) / 400;
  const int yoe = y - era * 400;                                    // [0, 399]
  const int doy = (153 * (m + (m > 2 ? -3 : 9)) + 2) / 5 + d - 1;   // [0, 365]
  const int doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;            // [0, 146096]
  return (int64_t)era * 146097 + doe - 719468;
}

LP_HD int ts_days_in_month(int y, int m) {
  if (m == 2) return (y % 4 == 0 && (y % 100 != 0 || y % 400 == 0)) ? 29 : 28;
  return 30 + ((m + (m >> 3)) & 1);
}

// the bytes of one line, read by offset: -1 at and behind the line's end. Device: aligned 16-byte
// loads (sig_ld16), the last one kept, so a walk that moves forward loads every block once.
struct TsBytes {
  const uint8_t* text;
  int64_t tbytes, start;
  int n;
#if defined(__HIP_DEVICE_COMPILE__)
  uint4 cur;
  int64_t cur_off;
#endif
  LP_HD TsBytes(const uint8_t* text_, int64_t tbytes_, int64_t start_, int n_)
      : text(text_), tbytes(tbytes_), start(start_), n(n_) {
#if defined(__HIP_DEVICE_COMPILE__)
    cur = make_uint4(0u, 0u, 0u, 0u);
    cur_off = -1;
#endif
  }
  LP_HD int at(int t) {
    if (t < 0 || t >= n) return -1;
#if defined(__HIP_DEVICE_COMPILE__)
    const int64_t a = start + t, off = a & ~int64_t(15);
    if (off != cur_off) {
      cur = sig_ld16(text, tbytes, off);
      cur_off = off;
    }
    const int j = (int)(a & 15);
    // (the four words are read first and the selects choose among values: a select among the
    // members themselves can become one load at a computed address, which puts `cur` into scratch)
    const uint32_t x0 = cur.x, x1 = cur.y, x2 = cur.z, x3 = cur.w;
    const uint32_t w = (j < 4) ? x0 : (j < 8) ? x1 : (j < 12) ? x2 : x3;
    return (int)((w >> (8 * (j & 3))) & 0xFFu);
#else
    return text[start + t];
#endif
  }
};

LP_HD bool ts_digit(int c) { return (unsigned)(c - '0') < 10u; }

// which offsets of the mandatory part take byte c (bit k: offset k)
LP_HD uint32_t ts_core_mask(int c) {
  constexpr uint32_t DIG = 0x6DB6Fu;      // 0-3, 5-6, 8-9, 11-12, 14-15, 17-18
  uint32_t m = ts_digit(c) ? DIG : 0u;
  m |= (c == '-' || c == '/') ? (1u << 4 | 1u << 7) : 0u;
  m |= (c == 'T' || c == ' ') ? (1u << 10) : 0u;
  m |= (c == ':') ? (1u << 13 | 1u << 16) : 0u;
  return m;
}

// epoch milliseconds of the stamp of the line text[start, start + n), or TS_NONE (text: 16-byte
// aligned on the device; never a byte before `text` or at / after text + tbytes).
//
// The mandatory part has a fixed length, so the leftmost match is the one that ends first: a
// shift-and walk keeps every open attempt in one word (bit k: an attempt has taken k + 1 bytes) and
// stops at the first one to take all TS_CORE bytes, or once no attempt is open and none may start.
// The low four bits of the last TS_CORE bytes ride along in two words, so the digits of the match
// are at hand when it completes and no byte is read twice: the walk only moves forward.
// Fraction and zone follow greedily, without backtracking; the fields are validated last, and a
// leftmost match with an invalid field means no stamp. `end`: the offset in the line of the first
// byte behind the stamp -- behind its zone, where it has one -- or 0 without a valid stamp.
LP_HD int64_t ts_scan_at(const uint8_t* __restrict__ text, int64_t tbytes, int64_t start, int n, int& end) {
  end = 0;
  if (start < 0) start = 0;
  if (start > tbytes) start = tbytes;
  if (n > TS_MAX_BYTES) n = TS_MAX_BYTES;
  if ((int64_t)n > tbytes - start) n = (int)(tbytes - start);
  if (n < TS_CORE) return TS_NONE;
  TsBytes B(text, tbytes, start, n);
  uint32_t open = 0u;
  uint64_t lo = 0u, hi = 0u;              // one nibble per byte walked, the latest in lo's low bits
  bool alnum = false;                     // the previous byte is [0-9A-Za-z]
  int p = -1;
  for (int t = 0; t < n; ++t) {
    if (t >= TS_MAX_START && open == 0u) break;
    const int c = B.at(t);
    open = ((open << 1) | ((t < TS_MAX_START && !alnum) ? 1u : 0u)) & ts_core_mask(c);
    hi = (hi << 4) | (lo >> 60);
    lo = (lo << 4) | (uint64_t)(c & 15);
    if (open & (1u << (TS_CORE - 1))) {
      p = t - (TS_CORE - 1);
      break;
    }
    alnum = ts_digit(c) || (unsigned)((c | 32) - 'a') < 26u;
  }
  if (p < 0) return TS_NONE;
  // digit at offset k of the match: nibble TS_CORE - 1 - k from the end of the history
  auto dig = [&](int k) {
    const int e = TS_CORE - 1 - k;
    return (int)((e < 16 ? lo >> (4 * e) : hi >> (4 * (e - 16))) & 15u);
  };
  auto two = [&](int k) { return dig(k) * 10 + dig(k + 1); };
  const int y = two(0) * 100 + two(2), mo = two(5), d = two(8), h = two(11), mi = two(14), s = two(17);
  int q = p + TS_CORE;
  int frac = 0;
  {
    const int c = B.at(q);
    if ((c == '.' || c == ',') && ts_digit(B.at(q + 1))) {
      int k = 0, scale = 100;
      for (++q; k < 9 && ts_digit(B.at(q)); ++k, ++q) {
        frac += (B.at(q) - '0') * scale;  // the first three digits; scale is 0 from the fourth on
        scale /= 10;
      }
    }
  }
  int zone = 0;                           // minutes east of UTC
  bool zone_ok = true;
  int qe = q;                             // the end of the match, zone included
  {
    const int c = B.at(q);
    if (c == 'Z') qe = q + 1;
    if (c == '+' || c == '-') {
      int r = q + 3;
      if (ts_digit(B.at(q + 1)) && ts_digit(B.at(q + 2))) {
        if (B.at(r) == ':') ++r;
        if (ts_digit(B.at(r)) && ts_digit(B.at(r + 1))) {
          const int zh = (B.at(q + 1) - '0') * 10 + (B.at(q + 2) - '0');
          const int zm = (B.at(r) - '0') * 10 + (B.at(r + 1) - '0');
          zone_ok = zh <= 23 && zm <= 59;
          zone = (c == '-' ? -1 : 1) * (zh * 60 + zm);
          qe = r + 2;
        }
      }
    }
  }
  if (!zone_ok || y < 1970 || mo < 1 || mo > 12 || d < 1 || d > ts_days_in_month(y, mo) || h > 23 || mi > 59 || s > 59)
    return TS_NONE;
  const int64_t secs = ts_days_from_civil(y, mo, d) * 86400 + h * 3600 + mi * 60 + s - (int64_t)zone * 60;
  end = qe;
  return secs * 1000 + frac;
}

LP_HD int64_t line_ts_at(const uint8_t* __restrict__ text, int64_t tbytes, int64_t start, int n) {
  int end;
  return ts_scan_at(text, tbytes, start, n, end);
}

// the stamp end of the line: the offset of the first byte behind its valid stamp (the end of the
// grammar's match: fraction and zone included), or 0 where line_ts_at gives TS_NONE -- an invalid
// stamp hides nothing (values.hip). At most TS_MAX_BYTES bytes of the line are read.
LP_HD int line_ts_span_at(const uint8_t* __restrict__ text, int64_t tbytes, int64_t start, int n) {
  int end;
  ts_scan_at(text, tbytes, start, n, end);
  return end;
}

}  // namespace lp
