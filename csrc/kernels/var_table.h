// Value table of the variants report (variants.hip): per (field, value) -- the group key
// val_key(signature, j) of a template's field and the hash of a token it held -- the number of
// lines, the first and the last of them, kept on the device across the chunks of a stream. The
// layout is gap_table.h's -- open addressing, linear probing, power-of-two capacity `cap`, cap + 1
// entries per column, entry `cap` the side slot of the one pair whose key is the empty marker --
// with a wider payload; the key is cell_table.h's cell_key(field, value). One source for the
// gfx950 kernels and their host twins.
//
// Columns as the caller initialises them (ops/kernels.py VarTable):
//   key      int64   GT_EMPTY in [0, cap); the side slot holds 0 until it is claimed, then GT_EMPTY
//   field    int64   0
//   value    int64   0
//   count    uint64  0
//   first    int64   INT64_MAX  (smallest global line number seen)
//   last     int64   INT64_MIN  (largest)
//   used     uint64[2]  0: occupied slots, and triples / rows that found no slot (always 0 while the
//                       caller keeps 2 * used <= cap)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cell_table.h"
#include "gap_table.h"
#include "lp_core.h"

namespace lp {

struct VarTab {
  int64_t* key;
  int64_t* field;
  int64_t* value;
  unsigned long long* count;
  long long* first;
  long long* last;
  unsigned long long* used;   // [2]
  int64_t cap;                // power of two
};

LP_HD bool vt_occupied(const VarTab& T, int64_t s) { return s < T.cap ? T.key[s] != GT_EMPTY : T.key[s] == GT_EMPTY; }

// slot of a key that is in the table (keys never change once written), or -1: gt_find on this layout
LP_HD int64_t vt_find(const VarTab& T, int64_t k) {
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

// is `field` in the set of fields to drop (a GapTab used as a set; without columns: the empty set)
LP_HD bool vt_skipped(const GapTab& skip, int64_t field) { return skip.key != nullptr && gt_find(skip, field) >= 0; }

}  // namespace lp
