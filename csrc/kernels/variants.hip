// Variants report: which values do the variable tokens of a line template take, and how often?
// k_line_vars walks every line once (var_core.h line_vars_at: template signature and the hashes of
// its fields' tokens in one pass), writes the signature of every line and the fields as compacted
// (line, val_key(signature, field), hash) triples -- 0..8 per line, on the block primitives of
// lp_block.h. The value table (var_table.h) counts the lines per (field, value) across launches:
//
//   k_var_fold      (field, value, global line) triples -> table, the fields of a skip set dropped
//   k_var_rows      occupied slots -> rows (field, value, count, first, last)
//   k_var_reinsert  rows of distinct (field, value) -> a fresh table (growth, purge)
//   k_var_winners   after the fold: the triples that hold their entry's first line (the lines whose
//                   text the host has to fetch as the value's example)
//
// log_parser_amd/variants.py drives them; log_parser_amd/golden.py variants is the specification.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

#include "lp_api.h"
#include "lp_block.h"
#include "lp_core.h"
#include "lp_host.h"
#include "var_core.h"
#include "var_table.h"

namespace lp {

namespace {
using ull = unsigned long long;
}

constexpr int VR_MAX_LINES = 2048;                  // lines per block at most
constexpr int VR_ROUND = 256;                       // lines per round: one per lane
constexpr int VR_STAGE = VR_ROUND * VAL_PER_LINE;   // triples of a round at most: 2048 x 20 B = 40 KiB of LDS

// A block owns `per_block` consecutive lines, one lane per line and round (k_line_vals' scheme). A
// round's lanes hold 0..8 triples each: an exclusive scan of the counts (block_excl_count) gives
// every lane its place in the round's LDS stage, the block reserves the round's output slots with
// ONE global atomic (block_reserve), and the stage is copied out coalesced.
__global__ __launch_bounds__(256) void k_line_vars(VarLinesArgs A, int per_block) {
  __shared__ int64_t l_field[VR_STAGE];
  __shared__ int64_t l_value[VR_STAGE];
  __shared__ int32_t l_line[VR_STAGE];
  __shared__ int s_wave[4];
  __shared__ int s_hit;
  __shared__ long long s_out;
  const int lane = threadIdx.x & 63;
  if (threadIdx.x == 0) s_hit = 0;
  const int64_t base = (int64_t)blockIdx.x * per_block;
  int hit_w = 0;                              // this wave's lines with a field (every lane holds it)
  for (int k0 = 0; k0 < per_block; k0 += VR_ROUND) {          // uniform trip count: shuffles and barriers are whole-block
    const int64_t i = base + k0 + (int)threadIdx.x;           // (k0 + threadIdx.x < per_block: a multiple of 256)
    const bool live = i < A.nl;
    VarList V;
    uint64_t sig = 0;
    if (live) {
      sig = line_vars_at(A.text, A.tbytes, A.ls[i], A.ll[i], V);
      A.sig[i] = (int64_t)sig;
    }
    const int c = __popc(V.mask);
    hit_w += __popcll(__ballot(c != 0));
    // exclusive scan of c over the round (its barrier also: the previous round's copy-out has read the stage)
    int total;
    int off = block_excl_count(c, s_wave, total);
    // stage: off + c <= total <= VR_STAGE
#pragma unroll
    for (int j = 0; j < VAL_PER_LINE; ++j) {
      if (V.mask & (1u << j)) {
        l_field[off] = (int64_t)val_key(sig, j);
        l_value[off] = (int64_t)V.v[j];
        l_line[off] = (int32_t)i;
        ++off;
      }
    }
    const int64_t o0 = block_reserve(A.cnt, total, &s_out);
    for (int j = threadIdx.x; j < total; j += VR_ROUND) {
      const int64_t o = o0 + j;
      if (o >= A.cap) break;                  // over capacity: counted above, the caller re-runs
      A.out_line[o] = l_line[j];
      A.out_field[o] = l_field[j];
      A.out_value[o] = l_value[j];
    }
    // (the next round's scan barrier stands between this copy-out and its writes of the stage and
    // of s_out; its write of s_wave comes after block_reserve's barrier of this round)
  }
  if (lane == 0 && hit_w) atomicAdd(&s_hit, hit_w);
  __syncthreads();
  if (threadIdx.x == 0 && s_hit) atomicAdd(A.cnt + 1, (ull)s_hit);
}

static void vr_check(const VarLinesArgs& A, const char* who) {
  const std::string w(who);
  if (A.nl < 0 || A.nl > 0x7fffffffll) throw std::runtime_error(w + ": too many lines for int32 line numbers");
  if (A.tbytes < 0) throw std::runtime_error(w + ": negative text size");
  if (A.cap < 0) throw std::runtime_error(w + ": negative capacity");
}

void line_vars_dev(const VarLinesArgs& A, uint64_t stream, int per_block) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  vr_check(A, "line_vars_dev");
  check_text_aligned(A.text, "line_vars_dev");
  if (A.nl <= 0) return;
  const LineGeom g = line_geom(A.nl, per_block, VR_MAX_LINES, "line_vars_dev");
  hipLaunchKernelGGL(k_line_vars, dim3(g.blocks), dim3(256), 0, st, A, g.per);
  LP_HIP_CHECK(hipGetLastError());
}

void line_vars_host(const VarLinesArgs& A) {
  vr_check(A, "line_vars_host");
  if (A.nl <= 0) return;
  // every worker walks the lines of its range; the ranges' triples are appended in line order
  struct Row {
    int32_t line;
    int64_t field;
    int64_t value;
  };
  const int T = std::max(1, host_threads());
  std::vector<std::vector<Row>> part(T);
  std::vector<int64_t> hits(T, 0);
  host_parallel(A.nl, 4096, [&](int t, int64_t a, int64_t b) {
    for (int64_t i = a; i < b; ++i) {
      VarList V;
      const uint64_t sig = line_vars_at(A.text, A.tbytes, A.ls[i], A.ll[i], V);
      A.sig[i] = (int64_t)sig;
      for (int j = 0; j < VAL_PER_LINE; ++j)
        if (V.mask & (1u << j)) part[t].push_back({(int32_t)i, (int64_t)val_key(sig, j), (int64_t)V.v[j]});
      if (V.mask) ++hits[t];
    }
  });
  int64_t o = 0, h = 0;
  for (int t = 0; t < T; ++t) {
    h += hits[t];
    for (const Row& r : part[t]) {
      if (o < A.cap) {
        A.out_line[o] = r.line;
        A.out_field[o] = r.field;
        A.out_value[o] = r.value;
      }
      ++o;
    }
  }
  A.cnt[0] += (ull)o;
  A.cnt[1] += (ull)h;
}

// ---- the value table

namespace {

// `cnt` triples of (field, value), the smallest ordinal of them `lo` and the largest `hi`, into
// slot s, the slot that gt_claim (gap_table.h) gave for cell_key(field, value). Everyone who
// flushes into a slot writes the same field and value: plain stores.
__device__ __forceinline__ void vt_apply(const VarTab& T, int64_t s, int64_t field, int64_t value, ull cnt, long long lo,
                                         long long hi) {
  T.field[s] = field;
  T.value[s] = value;
  atomicAdd(T.count + s, cnt);
  atomicMin(T.first + s, lo);
  atomicMax(T.last + s, hi);
}

}  // namespace

// A block owns `tile` consecutive triples (256..VT_TILE). A few values make most of an enumerable
// field, so the tile has few distinct (field, value): the block groups it in an LDS table
// (k_cell_fold's scheme: CAS on the key, bounded probes, LDS atomics for count, smallest and
// largest ordinal) and then issues one set of global atomics per distinct entry. A triple that
// finds no LDS slot within VT_LDS_PROBES probes and the pair whose key equals the empty marker go
// to the global table directly. The fields of `skip` are dropped: probed once per distinct LDS
// entry at flush time, once per triple on the direct path.
constexpr int VT_TILE = 2048;
constexpr int VT_BLOCKS = 512;
constexpr int VT_LDS_SLOTS = 1024;
constexpr int VT_LDS_PROBES = 8;

__global__ __launch_bounds__(256) void k_var_fold(VarTab T, GapTab skip, const int64_t* __restrict__ field,
                                                  const int64_t* __restrict__ value, const int64_t* __restrict__ ord,
                                                  int64_t n, int tile) {
  __shared__ ull lkey[VT_LDS_SLOTS];
  __shared__ long long lfld[VT_LDS_SLOTS];
  __shared__ long long lval[VT_LDS_SLOTS];
  __shared__ long long lmin[VT_LDS_SLOTS];
  __shared__ long long lmax[VT_LDS_SLOTS];
  __shared__ unsigned int lcnt[VT_LDS_SLOTS];
  __shared__ unsigned int s_fresh;
  if (threadIdx.x == 0) s_fresh = 0u;
  for (int j = threadIdx.x; j < VT_LDS_SLOTS; j += (int)blockDim.x) {
    lkey[j] = (ull)GT_EMPTY;
    lmin[j] = INT64_MAX;
    lmax[j] = INT64_MIN;
    lcnt[j] = 0u;
  }
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * tile;
  const int64_t end = base + tile < n ? base + tile : n;
  for (int64_t i = base + threadIdx.x; i < end; i += blockDim.x) {
    const int64_t f = field[i];
    const int64_t v = value[i];
    const int64_t k = cell_key(f, v);
    const long long g = ord[i];
    bool done = false;
    if (k != GT_EMPTY) {
      int h = (int)((gt_hash(k) >> 40) & (uint64_t)(VT_LDS_SLOTS - 1));   // (not the bits of the global slot)
      for (int p = 0; p < VT_LDS_PROBES && !done; ++p) {
        const ull was = atomicCAS(&lkey[h], (ull)GT_EMPTY, (ull)k);
        if (was == (ull)GT_EMPTY || was == (ull)k) {
          lfld[h] = f;                        // (the same values from every triple of the entry)
          lval[h] = v;
          atomicAdd(&lcnt[h], 1u);
          atomicMin(&lmin[h], g);
          atomicMax(&lmax[h], g);
          done = true;
        }
        h = (h + 1) & (VT_LDS_SLOTS - 1);
      }
    }
    if (!done && !vt_skipped(skip, f)) {
      const int64_t t = gt_claim(T, k, &s_fresh);
      if (t >= 0) vt_apply(T, t, f, v, 1ull, g, g);
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < VT_LDS_SLOTS; j += (int)blockDim.x) {
    const ull k = lkey[j];
    if (k == (ull)GT_EMPTY || vt_skipped(skip, lfld[j])) continue;
    const int64_t t = gt_claim(T, (int64_t)k, &s_fresh);
    if (t >= 0) vt_apply(T, t, lfld[j], lval[j], (ull)lcnt[j], lmin[j], lmax[j]);
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_fresh) atomicAdd(T.used, (ull)s_fresh);
}

// A block owns VW_SLOTS consecutive slots (the side slot included), a lane VW_ROUNDS of them; the
// block reserves its output rows with ONE global atomic (k_cell_rows' reservation).
constexpr int VW_ROUNDS = 8;
constexpr int VW_SLOTS = 256 * VW_ROUNDS;

__global__ __launch_bounds__(256) void k_var_rows(VarTab T, VarRows R, int64_t out_cap, ull* cnt) {
  __shared__ int s_wave[4];
  __shared__ long long s_out;
  const int64_t base = (int64_t)blockIdx.x * VW_SLOTS + (int)threadIdx.x;
  unsigned int occ = 0u;                      // bit r: slot base + 256 r is occupied
#pragma unroll
  for (int r = 0; r < VW_ROUNDS; ++r) {
    const int64_t s = base + 256 * r;
    if (s <= T.cap && vt_occupied(T, s)) occ |= 1u << r;
  }
  int total;
  const int off = block_excl_count(__popc(occ), s_wave, total);
  int64_t o = block_reserve(cnt, total, &s_out) + off;
#pragma unroll
  for (int r = 0; r < VW_ROUNDS; ++r) {
    if (!(occ & (1u << r))) continue;
    const int64_t s = base + 256 * r;
    if (o < out_cap) {                       // over capacity: counted, the caller sees cnt > out_cap
      R.field[o] = T.field[s];
      R.value[o] = T.value[s];
      R.count[o] = (int64_t)T.count[s];
      R.first[o] = T.first[s];
      R.last[o] = T.last[s];
    }
    ++o;
  }
}

// rows of DISTINCT (field, value) into a table that holds none of them: the claim is the only
// atomic (used[0] is not counted here: it is n, and the caller writes it)
__global__ __launch_bounds__(256) void k_var_reinsert(VarTab T, VarRows R, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t t = gt_claim(T, cell_key(R.field[i], R.value[i]), nullptr);
  if (t < 0) return;
  T.field[t] = R.field[i];
  T.value[t] = R.value[i];
  T.count[t] = (ull)R.count[i];
  T.first[t] = R.first[i];
  T.last[t] = R.last[i];
}

__global__ __launch_bounds__(256) void k_var_winners(VarTab T, const int64_t* __restrict__ field,
                                                     const int64_t* __restrict__ value, const int64_t* __restrict__ ord,
                                                     int64_t n, int64_t* __restrict__ out, ull* cnt) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool win = false;
  if (i < n) {
    const int64_t s = vt_find(T, cell_key(field[i], value[i]));
    win = s >= 0 && T.first[s] == ord[i];
  }
  const int64_t o = (int64_t)wave_list_append(__ballot(win), cnt);
  if (win && o < n) out[o] = i;              // (at most n winners: every triple is appended once)
}

static void vt_check(const VarTab& T, const char* who) {
  if (T.cap < 1 || (T.cap & (T.cap - 1)) != 0) throw std::runtime_error(std::string(who) + ": capacity must be a power of two");
  if (!T.key || !T.field || !T.value || !T.count || !T.first || !T.last || !T.used)
    throw std::runtime_error(std::string(who) + ": missing table column");
}

static void vt_check_skip(const GapTab& S, const char* who) {
  if (S.key && (S.cap < 1 || (S.cap & (S.cap - 1)) != 0))
    throw std::runtime_error(std::string(who) + ": the skip set's capacity must be a power of two");
}

static void vw_check(const VarRows& R, const char* who) {
  if (!R.field || !R.value || !R.count || !R.first || !R.last)
    throw std::runtime_error(std::string(who) + ": missing row column");
}

void var_fold_dev(const VarTab& T, const GapTab& skip, const int64_t* field, const int64_t* value, const int64_t* ord,
                  int64_t n, uint64_t stream, int tile) {
  vt_check(T, "var_fold_dev");
  vt_check_skip(skip, "var_fold_dev");
  if (n <= 0) return;
  if (tile <= 0) tile = (int)std::min<int64_t>(VT_TILE, std::max<int64_t>(256, (n / VT_BLOCKS + 255) / 256 * 256));
  if (tile < 256 || tile > VT_TILE || tile % 256) throw std::runtime_error("var_fold_dev: tile must be 256..2048, a multiple of 256");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_var_fold, dim3(launch_blocks(n, tile, "var_fold_dev")), dim3(256), 0, st, T, skip, field, value, ord, n,
                     tile);
  LP_HIP_CHECK(hipGetLastError());
}

void var_rows_dev(const VarTab& T, const VarRows& R, int64_t out_cap, unsigned long long* cnt, uint64_t stream) {
  vt_check(T, "var_rows_dev");
  if (out_cap > 0) vw_check(R, "var_rows_dev");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_var_rows, dim3(launch_blocks(T.cap + 1, VW_SLOTS, "var_rows_dev")), dim3(256), 0, st, T, R, out_cap, cnt);
  LP_HIP_CHECK(hipGetLastError());
}

void var_reinsert_dev(const VarTab& T, const VarRows& R, int64_t n, uint64_t stream) {
  vt_check(T, "var_reinsert_dev");
  if (n <= 0) return;
  vw_check(R, "var_reinsert_dev");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_var_reinsert, dim3(launch_blocks(n, 256, "var_reinsert_dev")), dim3(256), 0, st, T, R, n);
  LP_HIP_CHECK(hipGetLastError());
}

void var_winners_dev(const VarTab& T, const int64_t* field, const int64_t* value, const int64_t* ord, int64_t n,
                     int64_t* out, unsigned long long* cnt, uint64_t stream) {
  vt_check(T, "var_winners_dev");
  if (n <= 0) return;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_var_winners, dim3(launch_blocks(n, 256, "var_winners_dev")), dim3(256), 0, st, T, field, value, ord, n,
                     out, cnt);
  LP_HIP_CHECK(hipGetLastError());
}

// ---- host twins: the same table layout, one thread

static int64_t vt_claim_host(const VarTab& T, int64_t k) {
  if (k == GT_EMPTY) {
    if (T.key[T.cap] != GT_EMPTY) {
      T.key[T.cap] = GT_EMPTY;
      ++T.used[0];
    }
    return T.cap;
  }
  const int64_t mask = T.cap - 1;
  int64_t s = (int64_t)(gt_hash(k) & (uint64_t)mask);
  for (int64_t j = 0; j < T.cap; ++j) {
    if (T.key[s] == GT_EMPTY) {
      T.key[s] = k;
      ++T.used[0];
      return s;
    }
    if (T.key[s] == k) return s;
    s = (s + 1) & mask;
  }
  ++T.used[1];
  return -1;
}

void var_fold_host(const VarTab& T, const GapTab& skip, const int64_t* field, const int64_t* value, const int64_t* ord,
                   int64_t n) {
  vt_check(T, "var_fold_host");
  vt_check_skip(skip, "var_fold_host");
  for (int64_t i = 0; i < n; ++i) {
    if (vt_skipped(skip, field[i])) continue;
    const int64_t s = vt_claim_host(T, cell_key(field[i], value[i]));
    if (s < 0) continue;
    T.field[s] = field[i];
    T.value[s] = value[i];
    ++T.count[s];
    T.first[s] = std::min<long long>(T.first[s], ord[i]);
    T.last[s] = std::max<long long>(T.last[s], ord[i]);
  }
}

void var_rows_host(const VarTab& T, const VarRows& R, int64_t out_cap, unsigned long long* cnt) {
  vt_check(T, "var_rows_host");
  if (out_cap > 0) vw_check(R, "var_rows_host");
  unsigned long long o = *cnt;
  for (int64_t s = 0; s <= T.cap; ++s) {
    if (!vt_occupied(T, s)) continue;
    if ((int64_t)o < out_cap) {
      R.field[o] = T.field[s];
      R.value[o] = T.value[s];
      R.count[o] = (int64_t)T.count[s];
      R.first[o] = T.first[s];
      R.last[o] = T.last[s];
    }
    ++o;
  }
  *cnt = o;
}

void var_reinsert_host(const VarTab& T, const VarRows& R, int64_t n) {
  vt_check(T, "var_reinsert_host");
  if (n > 0) vw_check(R, "var_reinsert_host");
  const unsigned long long used = T.used[0];      // (not counted here either: the caller writes it)
  for (int64_t i = 0; i < n; ++i) {
    const int64_t t = vt_claim_host(T, cell_key(R.field[i], R.value[i]));
    T.used[0] = used;
    if (t < 0) continue;
    T.field[t] = R.field[i];
    T.value[t] = R.value[i];
    T.count[t] = (unsigned long long)R.count[i];
    T.first[t] = R.first[i];
    T.last[t] = R.last[i];
  }
}

void var_winners_host(const VarTab& T, const int64_t* field, const int64_t* value, const int64_t* ord, int64_t n,
                      int64_t* out, unsigned long long* cnt) {
  vt_check(T, "var_winners_host");
  unsigned long long o = *cnt;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t s = vt_find(T, cell_key(field[i], value[i]));
    if (s >= 0 && T.first[s] == ord[i]) out[o++] = i;
  }
  *cnt = o;
}

}  // namespace lp
