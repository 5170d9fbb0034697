// Cell table of the trends report (trends.hip): counts per (template signature, time bucket), kept
// on the device across the chunks of a stream. The layout is gap_table.h's -- open addressing,
// linear probing, power-of-two capacity `cap`, cap + 1 entries per column, entry `cap` the side
// slot of the one cell whose key is the empty marker -- with a wider payload. One source for the
// gfx950 kernels and their host twins.
//
// Columns as the caller initialises them (ops/kernels.py CellTable):
//   key      int64   GT_EMPTY in [0, cap); the side slot holds 0 until it is claimed, then GT_EMPTY
//   sig      int64   0          (the cell's template signature)
//   bucket   int64   0          (its bucket, CT_UNDATED for the template's undated lines)
//   count    uint64  0
//   first    int64   INT64_MAX  (smallest global line number seen)
//   used     uint64[2]  0: occupied slots, and pairs / rows that found no slot (always 0 while the
//                       caller keeps 2 * used <= cap)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gap_table.h"
#include "lp_core.h"
#include "ts_core.h"

namespace lp {

constexpr int64_t CT_UNDATED = INT64_MIN;      // the bucket of lines without an effective time
constexpr uint64_t CT_MIX = 0x9E3779B97F4A7C15ull;

struct CellTab {
  int64_t* key;
  int64_t* sig;
  int64_t* bucket;
  unsigned long long* count;
  long long* first;
  unsigned long long* used;   // [2]
  int64_t cap;                // power of two
};

// the 64-bit key of a cell (golden.trend_cell_key): sig + bucket * CT_MIX mod 2^64 -- for a fixed
// bucket a bijection of the signatures, so the cells of one bucket never collide; the slot comes
// from gt_hash of it
LP_HD int64_t cell_key(int64_t sig, int64_t bucket) {
  return (int64_t)((uint64_t)sig + (uint64_t)bucket * CT_MIX);
}

// the bucket of an effective time: floor(eff / W), also below zero (a stamp before 1970 UTC
// through a zone); W >= 1
LP_HD int64_t cell_bucket(int64_t eff, int64_t W) {
  if (eff == TS_NONE) return CT_UNDATED;
  int64_t q = eff / W;
  if (eff % W < 0) --q;
  return q;
}

LP_HD bool ct_occupied(const CellTab& T, int64_t s) { return s < T.cap ? T.key[s] != GT_EMPTY : T.key[s] == GT_EMPTY; }

}  // namespace lp
