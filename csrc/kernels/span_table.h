// Span table of the spans report (spans.hip): per id -- the key of key_core.h, FNV-1a-64 of a
// lowered token -- the whole span of its lines, kept on the device across the chunks of a stream:
// how many lines, the first and the last of them, the smallest and the largest effective time, the
// template signatures of the first and the last line, and the id's own bytes. The layout is
// gap_table.h's -- open addressing, linear probing, power-of-two capacity `cap`, cap + 1 entries per
// column, entry `cap` the side slot of the one key whose bit pattern is the empty marker -- with a
// wider payload. One source for the gfx950 kernels and their host twins.
//
// Columns as the caller initialises them (ops/kernels.py SpanTable):
//   key      int64   GT_EMPTY in [0, cap); the side slot holds 0 until it is claimed, then GT_EMPTY
//   count    uint64  0          (pairs: lines that hold the key)
//   first    int64   INT64_MAX  (smallest global line number)
//   last     int64   INT64_MIN  (largest)
//   tmin     int64   INT64_MAX  (smallest effective time of its timed lines)
//   tmax     int64   INT64_MIN  (largest; tmin > tmax: no line of the span has a time)
//   opens    int64   0          (signature of line `first`)
//   closes   int64   0          (signature of line `last`)
//   toklen   int32   0          (bytes of the token, 1..SPAN_TOK_BYTES)
//   tok      uint8[SPAN_TOK_BYTES]  0  (the lowered token of line `first`, zero padded; 8-byte aligned)
//   used     uint64[2]  0: occupied slots, and pairs / rows that found no slot or named no line
//                       (always 0 while the caller keeps 2 * used <= cap)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gap_table.h"
#include "key_core.h"
#include "lp_core.h"

namespace lp {

constexpr int SPAN_TOK_BYTES = KEY_MAX_LEN;      // 64
constexpr int SPAN_TOK_WORDS = SPAN_TOK_BYTES / 8;

struct SpanTab {
  int64_t* key;
  unsigned long long* count;
  long long* first;
  long long* last;
  long long* tmin;
  long long* tmax;
  int64_t* opens;
  int64_t* closes;
  int32_t* toklen;
  uint64_t* tok;              // SPAN_TOK_WORDS words per entry
  unsigned long long* used;   // [2]
  int64_t cap;                // power of two
};

// rows of a span table, or the rows to put into one
struct SpanRows {
  int64_t* key; int64_t* count; int64_t* first; int64_t* last; int64_t* tmin; int64_t* tmax;
  int64_t* opens; int64_t* closes; int32_t* toklen; uint64_t* tok;
};

LP_HD bool st_occupied(const SpanTab& T, int64_t s) { return s < T.cap ? T.key[s] != GT_EMPTY : T.key[s] == GT_EMPTY; }

// slot of a key that is in the table (keys never change once written), or -1: gt_find on this layout
LP_HD int64_t st_find(const SpanTab& T, int64_t k) {
  if (k == GT_EMPTY) return T.key[T.cap] == GT_EMPTY ? T.cap : -1;
  const int64_t mask = T.cap - 1;
  int64_t s = (int64_t)(gt_hash(k) & (uint64_t)mask);
  for (int64_t j = 0; j < T.cap; ++j) {
    const int64_t v = T.key[s];
    if (v == k) return s;
    if (v == GT_EMPTY) return -1;
    s = (s + 1) & mask;
  }
  return -1;
}

// Nested hash samples: a key is in sample `shift` when the top `shift` bits of gt_hash(key) are
// zero (0: every key; 64: the keys whose hash is 0), that is when its *level* -- the leading zero
// bits of the hash -- is at least `shift`. The table's slot uses the LOW bits of the same hash, so a
// sample fills a table as evenly as the whole does.
constexpr int SPAN_LEVELS = 65;   // levels 0..64

LP_HD int span_level(int64_t key) {
  const uint64_t h = gt_hash(key);
  if (h == 0) return 64;
#if defined(__HIP_DEVICE_COMPILE__)
  return __clzll((long long)h);
#else
  return __builtin_clzll(h);
#endif
}

LP_HD bool span_sampled(int64_t key, int shift) { return span_level(key) >= shift; }

// the token text[at, at + len) lowered into the SPAN_TOK_WORDS words of an entry, zero padded. The
// caller has checked 0 <= at, at + len <= tbytes, len <= SPAN_TOK_BYTES.
LP_HD void span_tok_store(uint64_t* __restrict__ dst, const uint8_t* __restrict__ text, int64_t at, int len) {
  for (int w = 0; w < SPAN_TOK_WORDS; ++w) {
    uint64_t v = 0;
    for (int b = 0; b < 8; ++b) {
      const int j = 8 * w + b;
      if (j < len) {
        const uint32_t c = text[at + j];
        v |= (uint64_t)(((c | 32u) - 'a' < 26u) ? (c | 32u) : c) << (8 * b);
      }
    }
    dst[w] = v;
  }
}

}  // namespace lp
