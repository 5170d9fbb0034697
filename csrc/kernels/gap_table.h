// Signature group table of the coverage-gap report (gap_table.hip): the grouping of (signature,
// ordinal) pairs that survives across launches -- chunks of one stream, documents of a corpus.
// Open addressing, linear probing, power-of-two capacity `cap`; every column has cap + 1 entries:
// [0, cap) is the probed range, entry `cap` is the side slot of the one signature whose bit pattern
// is the empty marker. One source for the gfx950 kernels and their host twins, as in gaps_core.h.
//
// Columns as the caller initialises them (ops/kernels.py GapTable):
//   key      int64   GT_EMPTY in [0, cap); the side slot holds 0 until it is claimed, then GT_EMPTY
//   count    uint64  0
//   first    int64   INT64_MAX  (smallest ordinal seen)
//   docs     int32   0          (documents the signature occurs in)
//   last_doc int32   -1         (largest document number seen)
//   used     uint64[2]  0: occupied slots, and pairs / rows that found no slot (always 0 while the
//                       caller keeps 2 * used <= cap; it raises when it reads anything else)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lp_core.h"

namespace lp {

constexpr int64_t GT_EMPTY = INT64_MIN;

struct GapTab {
  int64_t* key;
  unsigned long long* count;
  long long* first;
  int32_t* docs;
  int32_t* last_doc;
  unsigned long long* used;   // [2]
  int64_t cap;                // power of two
};

// the signatures are FNV-1a hashes whose low bits are weak (the last byte times an odd constant):
// the finaliser of MurmurHash3
LP_HD uint64_t gt_hash(int64_t sig) {
  uint64_t h = (uint64_t)sig;
  h ^= h >> 33;
  h *= 0xff51afd7ed558ccdull;
  h ^= h >> 33;
  h *= 0xc4ceb9fe1a85ec53ull;
  h ^= h >> 33;
  return h;
}

LP_HD bool gt_occupied(const GapTab& T, int64_t s) { return s < T.cap ? T.key[s] != GT_EMPTY : T.key[s] == GT_EMPTY; }

// slot of a signature that is in the table (keys never change once written), or -1
LP_HD int64_t gt_find(const GapTab& T, int64_t sig) {
  if (sig == GT_EMPTY) return T.key[T.cap] == GT_EMPTY ? T.cap : -1;
  const int64_t mask = T.cap - 1;
  int64_t s = (int64_t)(gt_hash(sig) & (uint64_t)mask);
  for (int64_t k = 0; k < T.cap; ++k) {
    const int64_t v = T.key[s];
    if (v == sig) return s;
    if (v == GT_EMPTY) return -1;
    s = (s + 1) & mask;
  }
  return -1;
}

#if defined(__HIPCC__)
// The slot of key `k` in the key column `key` of a table of this layout (cap + 1 entries), claimed
// if the key is new: 64-bit CAS on the key, linear probing, the side slot for the key that equals
// the empty marker. The load before the CAS is only a shortcut: a key never changes once it is
// written. -1 when every slot holds another key (the caller keeps the table at most half full, so
// this is never reached; it is counted in *overflow all the same and nothing is lost silently). A
// new slot is counted in *fresh (the block's LDS counter, or null: the caller knows the count):
// one atomic on the table's `used` per new slot would put every claim of a launch on one address.
__device__ __forceinline__ int64_t gt_claim(int64_t* key_col, int64_t cap, unsigned long long* overflow, int64_t k,
                                            unsigned int* fresh) {
  using ull = unsigned long long;
  ull* key = reinterpret_cast<ull*>(key_col);
  if (k == GT_EMPTY) {
    if (atomicCAS(key + cap, 0ull, (ull)GT_EMPTY) == 0ull && fresh) atomicAdd(fresh, 1u);
    return cap;
  }
  const int64_t mask = cap - 1;
  int64_t s = (int64_t)(gt_hash(k) & (uint64_t)mask);
  for (int64_t j = 0; j < cap; ++j) {
    ull v = __hip_atomic_load(key + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (v == (ull)GT_EMPTY) {
      v = atomicCAS(key + s, (ull)GT_EMPTY, (ull)k);
      if (v == (ull)GT_EMPTY) {
        if (fresh) atomicAdd(fresh, 1u);
        return s;
      }
    }
    if (v == (ull)k) return s;
    s = (s + 1) & mask;
  }
  atomicAdd(overflow, 1ull);
  return -1;
}

// on a table struct with the columns key, used and cap (GapTab, cell_table.h CellTab)
template <class Tab>
__device__ __forceinline__ int64_t gt_claim(const Tab& T, int64_t k, unsigned int* fresh) {
  return gt_claim(T.key, T.cap, T.used + 1, k, fresh);
}
#endif

}  // namespace lp
