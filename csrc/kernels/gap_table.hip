// Coverage-gap report across launches: the signature group table (gap_table.h). gaps.hip turns the
// uncovered error lines of one chunk or document into (line, signature) pairs; the kernels here
// fold such pairs, with an ordinal that orders them across chunks and documents, into a table that
// stays on the device: per signature its count, its smallest ordinal and the number of documents
// it occurs in (log_parser_amd/gapreport.py builds the stream, resident and corpus reports on it).
//
//   k_gap_fold      pairs -> table (atomic read-modify-writes on pre-initialised columns only)
//   k_gap_winners   after the fold: the pairs that hold their group's smallest ordinal (the lines
//                   whose text the host has to fetch as the group's example)
//   k_gap_rows      occupied slots -> rows (sig, count, first, docs, last_doc)
//   k_gap_reinsert  rows of distinct signatures -> a fresh table (growth)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>
#include <string>

#include "gap_table.h"
#include "lp_api.h"
#include "lp_block.h"
#include "lp_core.h"
#include "lp_host.h"

namespace lp {

namespace {

using ull = unsigned long long;

// `cnt` pairs of document `doc` with smallest ordinal `ord` into slot s. The old value of the
// atomicMax tells the first arrival of a document apart (one document per launch, document
// numbers never decrease from launch to launch).
__device__ __forceinline__ void gt_apply(const GapTab& T, int64_t s, ull cnt, long long ord, int doc) {
  atomicAdd(T.count + s, cnt);
  atomicMin(T.first + s, ord);
  if (atomicMax(T.last_doc + s, doc) < doc) atomicAdd(T.docs + s, 1);
}

}  // namespace

// A block owns `tile` consecutive pairs (256..GT_TILE). Hot templates put most pairs of a log on a handful of
// signatures, and global atomics on one address serialise: the block first groups its pairs in an
// LDS table (signature -> count, smallest ordinal; LDS atomics) and then issues one set of global
// atomics per distinct signature. A pair that finds no LDS slot within GT_LDS_PROBES probes -- more
// distinct signatures in the tile than the table takes -- and the signature that equals the empty
// marker go to the global table directly.
constexpr int GT_TILE = 2048;          // the largest tile
constexpr int GT_BLOCKS = 512;         // a launch is cut into about this many tiles (of 256 pairs at least)
constexpr int GT_LDS_SLOTS = 1024;
constexpr int GT_LDS_PROBES = 8;

__global__ __launch_bounds__(256) void k_gap_fold(GapTab T, const int64_t* __restrict__ sig,
                                                  const int64_t* __restrict__ ord, int64_t n, int doc, int tile) {
  __shared__ ull lkey[GT_LDS_SLOTS];
  __shared__ long long lmin[GT_LDS_SLOTS];
  __shared__ unsigned int lcnt[GT_LDS_SLOTS];
  __shared__ unsigned int s_fresh;
  if (threadIdx.x == 0) s_fresh = 0u;
  for (int j = threadIdx.x; j < GT_LDS_SLOTS; j += (int)blockDim.x) {
    lkey[j] = (ull)GT_EMPTY;
    lmin[j] = INT64_MAX;
    lcnt[j] = 0u;
  }
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * tile;
  const int64_t end = base + tile < n ? base + tile : n;
  for (int64_t i = base + threadIdx.x; i < end; i += blockDim.x) {
    const int64_t s = sig[i];
    const long long o = ord[i];
    bool done = false;
    if (s != GT_EMPTY) {
      int h = (int)((gt_hash(s) >> 40) & (uint64_t)(GT_LDS_SLOTS - 1));   // (not the bits of the global slot)
      for (int p = 0; p < GT_LDS_PROBES && !done; ++p) {
        const ull v = atomicCAS(&lkey[h], (ull)GT_EMPTY, (ull)s);
        if (v == (ull)GT_EMPTY || v == (ull)s) {
          atomicAdd(&lcnt[h], 1u);
          atomicMin(&lmin[h], o);
          done = true;
        }
        h = (h + 1) & (GT_LDS_SLOTS - 1);
      }
    }
    if (!done) {
      const int64_t g = gt_claim(T, s, &s_fresh);
      if (g >= 0) gt_apply(T, g, 1ull, o, doc);
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < GT_LDS_SLOTS; j += (int)blockDim.x) {
    const ull k = lkey[j];
    if (k == (ull)GT_EMPTY) continue;
    const int64_t g = gt_claim(T, (int64_t)k, &s_fresh);
    if (g >= 0) gt_apply(T, g, (ull)lcnt[j], lmin[j], doc);
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_fresh) atomicAdd(T.used, (ull)s_fresh);
}

// one lane per pair; the winners of a wave reserve their output slots with one atomic (wave_list_append)
__global__ __launch_bounds__(256) void k_gap_winners(GapTab T, const int64_t* __restrict__ sig,
                                                     const int64_t* __restrict__ ord, int64_t n,
                                                     int64_t* __restrict__ out, ull* cnt) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool win = false;
  if (i < n) {
    const int64_t s = gt_find(T, sig[i]);
    win = s >= 0 && T.first[s] == ord[i];
  }
  const int64_t o = (int64_t)wave_list_append(__ballot(win), cnt);
  if (win && o < n) out[o] = i;              // (at most n winners: every pair is appended once)
}

// one lane per slot, the side slot included
__global__ __launch_bounds__(256) void k_gap_rows(GapTab T, int64_t* __restrict__ o_sig, int64_t* __restrict__ o_count,
                                                  int64_t* __restrict__ o_first, int32_t* __restrict__ o_docs,
                                                  int32_t* __restrict__ o_last, int64_t out_cap, ull* cnt) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool occ = s <= T.cap && gt_occupied(T, s);
  const int64_t o = (int64_t)wave_list_append(__ballot(occ), cnt);
  if (occ && o < out_cap) {                  // over capacity: counted, the caller sees cnt > out_cap
    o_sig[o] = s < T.cap ? T.key[s] : GT_EMPTY;
    o_count[o] = (int64_t)T.count[s];
    o_first[o] = T.first[s];
    o_docs[o] = T.docs[s];
    o_last[o] = T.last_doc[s];
  }
}

// rows of DISTINCT signatures into a table that holds none of them: the claim is the only atomic
// (used[0] is not counted here: it is n, and the caller writes it)
__global__ __launch_bounds__(256) void k_gap_reinsert(GapTab T, const int64_t* __restrict__ r_sig,
                                                      const int64_t* __restrict__ r_count,
                                                      const int64_t* __restrict__ r_first,
                                                      const int32_t* __restrict__ r_docs,
                                                      const int32_t* __restrict__ r_last, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t g = gt_claim(T, r_sig[i], nullptr);
  if (g < 0) return;
  T.count[g] = (ull)r_count[i];
  T.first[g] = r_first[i];
  T.docs[g] = r_docs[i];
  T.last_doc[g] = r_last[i];
}

static void gt_check(const GapTab& T, const char* who) {
  if (T.cap < 1 || (T.cap & (T.cap - 1)) != 0) throw std::runtime_error(std::string(who) + ": capacity must be a power of two");
  if (!T.key || !T.count || !T.first || !T.docs || !T.last_doc || !T.used)
    throw std::runtime_error(std::string(who) + ": missing table column");
}

void gap_fold_dev(const GapTab& T, const int64_t* sig, const int64_t* ord, int64_t n, int doc, uint64_t stream,
                  int tile) {
  gt_check(T, "gap_fold_dev");
  if (n <= 0) return;
  // a chunk's pairs are few (thousands): tiles of GT_TILE would leave most CUs idle while each block
  // walks its tile in rounds of dependent atomics, so small launches get small tiles
  if (tile <= 0) tile = (int)std::min<int64_t>(GT_TILE, std::max<int64_t>(256, (n / GT_BLOCKS + 255) / 256 * 256));
  if (tile < 256 || tile > GT_TILE || tile % 256) throw std::runtime_error("gap_fold_dev: tile must be 256..2048, a multiple of 256");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_gap_fold, dim3(launch_blocks(n, tile, "gap_fold_dev")), dim3(256), 0, st, T, sig, ord, n, doc, tile);
  LP_HIP_CHECK(hipGetLastError());
}

void gap_winners_dev(const GapTab& T, const int64_t* sig, const int64_t* ord, int64_t n, int64_t* out,
                     unsigned long long* cnt, uint64_t stream) {
  gt_check(T, "gap_winners_dev");
  if (n <= 0) return;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_gap_winners, dim3(launch_blocks(n, 256, "gap_winners_dev")), dim3(256), 0, st, T, sig, ord, n, out, cnt);
  LP_HIP_CHECK(hipGetLastError());
}

void gap_rows_dev(const GapTab& T, const GapRows& R, int64_t out_cap, unsigned long long* cnt, uint64_t stream) {
  gt_check(T, "gap_rows_dev");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_gap_rows, dim3(launch_blocks(T.cap + 1, 256, "gap_rows_dev")), dim3(256), 0, st, T, R.sig, R.count,
                     R.first, R.docs, R.last_doc, out_cap, cnt);
  LP_HIP_CHECK(hipGetLastError());
}

void gap_reinsert_dev(const GapTab& T, const GapRows& R, int64_t n, uint64_t stream) {
  gt_check(T, "gap_reinsert_dev");
  if (n <= 0) return;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_gap_reinsert, dim3(launch_blocks(n, 256, "gap_reinsert_dev")), dim3(256), 0, st, T, R.sig, R.count,
                     R.first, R.docs, R.last_doc, n);
  LP_HIP_CHECK(hipGetLastError());
}

// ---- host twins: the same table layout, one thread (the table work of a chunk is small next to
// the matchers')

static int64_t gt_claim_host(const GapTab& T, int64_t sig) {
  if (sig == GT_EMPTY) {
    if (T.key[T.cap] != GT_EMPTY) {
      T.key[T.cap] = GT_EMPTY;
      ++T.used[0];
    }
    return T.cap;
  }
  const int64_t mask = T.cap - 1;
  int64_t s = (int64_t)(gt_hash(sig) & (uint64_t)mask);
  for (int64_t k = 0; k < T.cap; ++k) {
    if (T.key[s] == GT_EMPTY) {
      T.key[s] = sig;
      ++T.used[0];
      return s;
    }
    if (T.key[s] == sig) return s;
    s = (s + 1) & mask;
  }
  ++T.used[1];
  return -1;
}

void gap_fold_host(const GapTab& T, const int64_t* sig, const int64_t* ord, int64_t n, int doc) {
  gt_check(T, "gap_fold_host");
  for (int64_t i = 0; i < n; ++i) {
    const int64_t s = gt_claim_host(T, sig[i]);
    if (s < 0) continue;
    ++T.count[s];
    T.first[s] = std::min<long long>(T.first[s], ord[i]);
    if (T.last_doc[s] < doc) {
      T.last_doc[s] = doc;
      ++T.docs[s];
    }
  }
}

void gap_winners_host(const GapTab& T, const int64_t* sig, const int64_t* ord, int64_t n, int64_t* out,
                      unsigned long long* cnt) {
  gt_check(T, "gap_winners_host");
  unsigned long long o = *cnt;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t s = gt_find(T, sig[i]);
    if (s >= 0 && T.first[s] == ord[i] && (int64_t)o < n) out[o++] = i;
  }
  *cnt = o;
}

void gap_rows_host(const GapTab& T, const GapRows& R, int64_t out_cap, unsigned long long* cnt) {
  gt_check(T, "gap_rows_host");
  unsigned long long o = *cnt;
  for (int64_t s = 0; s <= T.cap; ++s) {
    if (!gt_occupied(T, s)) continue;
    if ((int64_t)o < out_cap) {
      R.sig[o] = s < T.cap ? T.key[s] : GT_EMPTY;
      R.count[o] = (int64_t)T.count[s];
      R.first[o] = T.first[s];
      R.docs[o] = T.docs[s];
      R.last_doc[o] = T.last_doc[s];
    }
    ++o;
  }
  *cnt = o;
}

void gap_reinsert_host(const GapTab& T, const GapRows& R, int64_t n) {
  gt_check(T, "gap_reinsert_host");
  const unsigned long long used = T.used[0];      // (not counted here either: the caller writes it)
  for (int64_t i = 0; i < n; ++i) {
    const int64_t g = gt_claim_host(T, R.sig[i]);
    T.used[0] = used;
    if (g < 0) continue;
    T.count[g] = (unsigned long long)R.count[i];
    T.first[g] = R.first[i];
    T.docs[g] = R.docs[i];
    T.last_doc[g] = R.last_doc[i];
  }
}

}  // namespace lp
