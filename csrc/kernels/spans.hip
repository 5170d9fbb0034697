// Spans report: the lifetimes of the ids of a log. k_span_keys walks every line ONCE for the three
// things the report needs of it -- its stamp (ts_core.h), its template signature (gaps_core.h) and
// its keys with their places (key_core.h) -- and writes signature and stamp per line and the keys of
// the current hash sample (span_table.h span_sampled) as compacted (line, key, place) triples, 0..8
// per line, on the block primitives of lp_block.h. The span table (span_table.h) keeps a whole span
// per key across launches:
//
//   k_span_fold      (line, key) pairs -> count, first / last line, smallest / largest effective time
//   k_span_ends      after the fold: the pairs that hold their span's first line write its opening
//                    signature and the token's bytes, those that hold its last line the closing one
//   k_span_rows      occupied slots -> rows
//   k_span_reinsert  rows of distinct keys -> a fresh table (growth, purge)
//
// log_parser_amd/spans.py drives them; log_parser_amd/golden.py spans is the specification.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

#include "gaps_core.h"
#include "key_core.h"
#include "lp_api.h"
#include "lp_block.h"
#include "lp_core.h"
#include "lp_host.h"
#include "span_table.h"
#include "ts_core.h"

namespace lp {

namespace {
using ull = unsigned long long;
}

constexpr int SK_MAX_LINES = 2048;                  // lines per block at most
constexpr int SK_ROUND = 256;                       // lines per round: one per lane
constexpr int SK_STAGE = SK_ROUND * KEY_PER_LINE;   // triples of a round at most: 2048 x 16 B = 32 KiB of LDS

// Stamp, signature and keys of the line text[start, start + n) (text: 16-byte aligned on the
// device). The stamp comes first, as in k_line_stamps: its walk ends within the line's first 67
// bytes. Then ONE forward pass, sig_step and key_step_at side by side on the loads of line_keys_at
// -- aligned 16-byte loads one block ahead; never a byte before `text` or at / after text + tbytes.
// A token still open at the end of the walk -- the end of the line, or byte SIG_MAX_BYTES -- ends
// there.
LP_HD uint64_t line_span_at(const uint8_t* __restrict__ text, int64_t tbytes, int64_t start, int n, int min_len,
                            int64_t& ts, KeyList& K, KeyPosList& P) {
  if (start < 0) start = 0;
  if (start > tbytes) start = tbytes;
  ts = line_ts_at(text, tbytes, start, n);
  if (n > SIG_MAX_BYTES) n = SIG_MAX_BYTES;
  if ((int64_t)n > tbytes - start) n = (int)(tbytes - start);
  if (n < 0) n = 0;
  SigState S;
  KeyState Y;
#if defined(__HIP_DEVICE_COMPILE__)
  if (n > 0) {
    const int sh = (int)(start & 15);
    int64_t off = start - sh;
    uint4 cur = sig_ld16(text, tbytes, off);
    for (int t0 = -sh; t0 < n; t0 += 16) {
      off += 16;
      const uint4 nxt = t0 + 16 < n ? sig_ld16(text, tbytes, off) : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int t = t0 + j;
        const uint32_t w = (j < 4) ? cur.x : (j < 8) ? cur.y : (j < 12) ? cur.z : cur.w;
        const uint32_t c = (w >> (8 * (j & 3))) & 0xFFu;
        const bool on = (t >= 0) & (t < n);
        key_step_at(Y, K, P, c, t, on, min_len);
        sig_step(S, c, on);
      }
      cur = nxt;
    }
  }
#else
  for (int t = 0; t < n; ++t) {
    key_step_at(Y, K, P, text[start + t], t, true, min_len);
    sig_step(S, text[start + t], true);
  }
#endif
  if (key_qualifies(Y, min_len)) key_insert_at(K, P, (int64_t)Y.h, key_pos_pack(n - (int)Y.len, Y.len));
  return sig_finish(S);
}

// A block owns `per_block` consecutive lines, one lane per line and round (k_line_keys' scheme). A
// round's lanes hold 0..8 sampled triples each: an exclusive scan of the counts (block_excl_count)
// gives every lane its place in the round's LDS stage, the block reserves the round's output slots
// with ONE global atomic (block_reserve), and the stage is copied out coalesced. The sample test
// comes after the line's first KEY_PER_LINE distinct keys are chosen: a line means the same under
// every shift.
__global__ __launch_bounds__(256) void k_span_keys(SpanLinesArgs A, int per_block) {
  __shared__ int64_t l_key[SK_STAGE];
  __shared__ int32_t l_line[SK_STAGE];
  __shared__ int32_t l_tok[SK_STAGE];
  __shared__ int s_wave[4];
  __shared__ int s_hit;
  __shared__ unsigned int s_lvl[SPAN_LEVELS];
  __shared__ long long s_out;
  const int lane = threadIdx.x & 63;
  if (threadIdx.x == 0) s_hit = 0;
  if (threadIdx.x < SPAN_LEVELS) s_lvl[threadIdx.x] = 0u;    // (the first round's scan barrier stands before its use)
  const int64_t base = (int64_t)blockIdx.x * per_block;
  int hit_w = 0;                              // this wave's lines with a triple (every lane holds it)
  for (int k0 = 0; k0 < per_block; k0 += SK_ROUND) {          // uniform trip count: shuffles and barriers are whole-block
    const int64_t i = base + k0 + (int)threadIdx.x;           // (k0 + threadIdx.x < per_block: a multiple of 256)
    KeyList K;
    KeyPosList P;
    if (i < A.nl) {
      int64_t ts;
      A.sig[i] = (int64_t)line_span_at(A.text, A.tbytes, A.ls[i], A.ll[i], A.min_len, ts, K, P);
      A.ts[i] = ts;
    }
    uint32_t keep = 0u;                       // bit j: slot j is in the sample
    int deepest = -1;                         // the largest level of the line's keys
#pragma unroll
    for (int j = 0; j < KEY_PER_LINE; ++j) {
      const int lv = j < K.n ? span_level(K.k[j]) : -1;
      if (lv >= A.shift) keep |= 1u << j;     // (shift >= 0: an empty slot is never kept)
      deepest = lv > deepest ? lv : deepest;
    }
    const int c = __popc(keep);
    hit_w += __popcll(__ballot(c != 0));
    // exclusive scan of c over the round (its barrier also: the previous round's copy-out has read the stage)
    int total;
    int off = block_excl_count(c, s_wave, total);
    if (c != 0 && A.lvl) atomicAdd(&s_lvl[deepest], 1u);      // (c != 0: deepest >= shift >= 0)
    // stage: off + c <= total <= SK_STAGE
#pragma unroll
    for (int j = 0; j < KEY_PER_LINE; ++j) {
      if (keep & (1u << j)) {
        l_key[off] = K.k[j];
        l_line[off] = (int32_t)i;
        l_tok[off] = P.p[j];
        ++off;
      }
    }
    const int64_t o0 = block_reserve(A.cnt, total, &s_out);
    for (int j = threadIdx.x; j < total; j += SK_ROUND) {
      const int64_t o = o0 + j;
      if (o >= A.cap) break;                  // over capacity: counted above, the caller re-runs
      A.out_line[o] = l_line[j];
      A.out_key[o] = l_key[j];
      A.out_tok[o] = l_tok[j];
    }
    // (the next round's scan barrier stands between this copy-out and its writes of the stage and
    // of s_out; its write of s_wave comes after block_reserve's barrier of this round)
  }
  if (lane == 0 && hit_w) atomicAdd(&s_hit, hit_w);
  __syncthreads();
  if (threadIdx.x == 0 && s_hit) atomicAdd(A.cnt + 1, (ull)s_hit);
  if (A.lvl && threadIdx.x < SPAN_LEVELS && s_lvl[threadIdx.x]) atomicAdd(A.lvl + threadIdx.x, (ull)s_lvl[threadIdx.x]);
}

static void sk_check(const SpanLinesArgs& A, const char* who) {
  const std::string w(who);
  if (A.min_len < KEY_MIN_LEN_LO || A.min_len > KEY_MAX_LEN)
    throw std::runtime_error(w + ": min_len must be " + std::to_string(KEY_MIN_LEN_LO) + ".." + std::to_string(KEY_MAX_LEN));
  if (A.shift < 0 || A.shift > 64) throw std::runtime_error(w + ": shift must be 0..64");
  if (A.nl < 0 || A.nl > 0x7fffffffll) throw std::runtime_error(w + ": too many lines for int32 line numbers");
  if (A.tbytes < 0) throw std::runtime_error(w + ": negative text size");
  if (A.cap < 0) throw std::runtime_error(w + ": negative capacity");
}

void span_keys_dev(const SpanLinesArgs& A, uint64_t stream, int per_block) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  sk_check(A, "span_keys_dev");
  check_text_aligned(A.text, "span_keys_dev");
  if (A.nl <= 0) return;
  const LineGeom g = line_geom(A.nl, per_block, SK_MAX_LINES, "span_keys_dev");
  hipLaunchKernelGGL(k_span_keys, dim3(g.blocks), dim3(256), 0, st, A, g.per);
  LP_HIP_CHECK(hipGetLastError());
}

void span_keys_host(const SpanLinesArgs& A) {
  sk_check(A, "span_keys_host");
  if (A.nl <= 0) return;
  // every worker walks the lines of its range; the ranges' triples are appended in line order
  struct Row {
    int32_t line;
    int64_t key;
    int32_t tok;
  };
  const int T = std::max(1, host_threads());
  std::vector<std::vector<Row>> part(T);
  std::vector<int64_t> hits(T, 0);
  std::vector<std::vector<int64_t>> lvl(T, std::vector<int64_t>(SPAN_LEVELS, 0));
  host_parallel(A.nl, 4096, [&](int t, int64_t a, int64_t b) {
    for (int64_t i = a; i < b; ++i) {
      KeyList K;
      KeyPosList P;
      int64_t ts;
      A.sig[i] = (int64_t)line_span_at(A.text, A.tbytes, A.ls[i], A.ll[i], A.min_len, ts, K, P);
      A.ts[i] = ts;
      int deepest = -1;
      for (int j = 0; j < K.n; ++j) {
        const int lv = span_level(K.k[j]);
        if (lv < A.shift) continue;
        part[t].push_back({(int32_t)i, K.k[j], P.p[j]});
        deepest = std::max(deepest, lv);
      }
      if (deepest >= 0) {
        ++hits[t];
        ++lvl[t][deepest];
      }
    }
  });
  int64_t o = 0, h = 0;
  for (int t = 0; t < T; ++t) {
    h += hits[t];
    if (A.lvl)
      for (int m = 0; m < SPAN_LEVELS; ++m) A.lvl[m] += (ull)lvl[t][m];
    for (const Row& r : part[t]) {
      if (o < A.cap) {
        A.out_line[o] = r.line;
        A.out_key[o] = r.key;
        A.out_tok[o] = r.tok;
      }
      ++o;
    }
  }
  A.cnt[0] += (ull)o;
  A.cnt[1] += (ull)h;
}

// ---- the span table

// One lane per pair; every step is a plain 64-bit global atomic on the key's slot. In an id-heavy
// log nearly every key of a tile is distinct, so grouping a tile in LDS first (k_gap_fold) would
// find little to merge. A pair whose line is not one of the piece's `nl` lines is counted as lost.
__global__ __launch_bounds__(256) void k_span_fold(SpanTab T, SpanPairs X) {
  __shared__ unsigned int s_fresh;
  if (threadIdx.x == 0) s_fresh = 0u;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < X.n) {
    const int64_t x = X.line[i];
    if (x < 0 || x >= X.nl) {
      atomicAdd(T.used + 1, 1ull);
    } else {
      const int64_t s = gt_claim(T, X.key[i], &s_fresh);
      if (s >= 0) {
        const long long g = X.line_base + x;
        atomicAdd(T.count + s, 1ull);
        atomicMin(T.first + s, g);
        atomicMax(T.last + s, g);
        const long long e = X.eff[x];
        if (e != TS_NONE) {
          atomicMin(T.tmin + s, e);
          atomicMax(T.tmax + s, e);
        }
      }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_fresh) atomicAdd(T.used, (ull)s_fresh);
}

// what a pair writes once the fold of its launch is complete (both: device and host)
LP_HD void span_end_pair(const SpanTab& T, const SpanPairs& X, int64_t i) {
  const int64_t x = X.line[i];
  if (x < 0 || x >= X.nl) return;
  const int64_t s = st_find(T, X.key[i]);
  if (s < 0) return;
  const long long g = X.line_base + x;
  if (T.first[s] == g) {
    // a line holds a key once: this pair is the slot's only writer of these columns, in this launch
    // and in every other (no later line comes before it)
    const int32_t p = X.tok[i];
    const int len = (int)(p >> KEY_POS_LEN_SHIFT);
    int64_t at = X.ls[x];
    if (at < 0) at = 0;                       // (the clamp of line_span_at)
    at += p & KEY_POS_OFF_MASK;
    T.opens[s] = X.sig[x];
    if (len >= 1 && len <= SPAN_TOK_BYTES && at + len <= X.tbytes) {
      T.toklen[s] = len;
      span_tok_store(T.tok + s * SPAN_TOK_WORDS, X.text, at, len);
    }
  }
  if (T.last[s] == g) T.closes[s] = X.sig[x];
}

// A second launch on the fold's stream: `first` and `last` are final only once every block of the
// fold has finished.
__global__ __launch_bounds__(256) void k_span_ends(SpanTab T, SpanPairs X) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < X.n) span_end_pair(T, X, i);
}

LP_HD void span_row_out(const SpanTab& T, int64_t s, const SpanRows& R, int64_t o) {
  R.key[o] = s < T.cap ? T.key[s] : GT_EMPTY;
  R.count[o] = (int64_t)T.count[s];
  R.first[o] = T.first[s];
  R.last[o] = T.last[s];
  R.tmin[o] = T.tmin[s];
  R.tmax[o] = T.tmax[s];
  R.opens[o] = T.opens[s];
  R.closes[o] = T.closes[s];
  R.toklen[o] = T.toklen[s];
  for (int w = 0; w < SPAN_TOK_WORDS; ++w) R.tok[o * SPAN_TOK_WORDS + w] = T.tok[s * SPAN_TOK_WORDS + w];
}

LP_HD void span_row_in(const SpanTab& T, int64_t s, const SpanRows& R, int64_t i) {
  T.count[s] = (ull)R.count[i];
  T.first[s] = R.first[i];
  T.last[s] = R.last[i];
  T.tmin[s] = R.tmin[i];
  T.tmax[s] = R.tmax[i];
  T.opens[s] = R.opens[i];
  T.closes[s] = R.closes[i];
  T.toklen[s] = R.toklen[i];
  for (int w = 0; w < SPAN_TOK_WORDS; ++w) T.tok[s * SPAN_TOK_WORDS + w] = R.tok[i * SPAN_TOK_WORDS + w];
}

// the slot is occupied and its key is in sample `shift` (0: every occupied slot)
LP_HD bool st_listed(const SpanTab& T, int64_t s, int shift) {
  return st_occupied(T, s) && (shift <= 0 || span_sampled(s < T.cap ? T.key[s] : GT_EMPTY, shift));
}

// A block owns SW_SLOTS consecutive slots (the side slot included), a lane SW_ROUNDS of them; the
// block reserves its output rows with ONE global atomic (k_var_rows' reservation). Only the rows of
// sample `shift` are written and counted: the purge reads the table through its own filter.
constexpr int SW_ROUNDS = 8;
constexpr int SW_SLOTS = 256 * SW_ROUNDS;

__global__ __launch_bounds__(256) void k_span_rows(SpanTab T, SpanRows R, int64_t out_cap, ull* cnt, int shift) {
  __shared__ int s_wave[4];
  __shared__ long long s_out;
  const int64_t base = (int64_t)blockIdx.x * SW_SLOTS + (int)threadIdx.x;
  unsigned int occ = 0u;                      // bit r: slot base + 256 r is occupied
#pragma unroll
  for (int r = 0; r < SW_ROUNDS; ++r) {
    const int64_t s = base + 256 * r;
    if (s <= T.cap && st_listed(T, s, shift)) occ |= 1u << r;
  }
  int total;
  const int off = block_excl_count(__popc(occ), s_wave, total);
  int64_t o = block_reserve(cnt, total, &s_out) + off;
#pragma unroll
  for (int r = 0; r < SW_ROUNDS; ++r) {
    if (!(occ & (1u << r))) continue;
    if (o < out_cap) span_row_out(T, base + 256 * r, R, o);   // over capacity: counted, the caller sees cnt > out_cap
    ++o;
  }
}

// rows of DISTINCT keys into a table that holds none of them: the claim is the only atomic
// (used[0] is not counted here: it is n, and the caller writes it)
__global__ __launch_bounds__(256) void k_span_reinsert(SpanTab T, SpanRows R, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t s = gt_claim(T, R.key[i], nullptr);
  if (s >= 0) span_row_in(T, s, R, i);
}

static void st_check(const SpanTab& T, const char* who) {
  if (T.cap < 1 || (T.cap & (T.cap - 1)) != 0) throw std::runtime_error(std::string(who) + ": capacity must be a power of two");
  if (!T.key || !T.count || !T.first || !T.last || !T.tmin || !T.tmax || !T.opens || !T.closes || !T.toklen || !T.tok ||
      !T.used)
    throw std::runtime_error(std::string(who) + ": missing table column");
  if (((uintptr_t)T.tok & 7) != 0) throw std::runtime_error(std::string(who) + ": the token column must be 8-byte aligned");
}

static void sp_check(const SpanPairs& X, const char* who) {
  const std::string w(who);
  if (X.n < 0 || X.nl < 0 || X.nl > 0x7fffffffll) throw std::runtime_error(w + ": bad pair or line count");
  if (X.tbytes < 0) throw std::runtime_error(w + ": negative text size");
  if (X.n > 0 && (!X.line || !X.key || !X.tok || !X.sig || !X.eff || !X.text || !X.ls))
    throw std::runtime_error(w + ": missing pair column");
}

static void sw_check(const SpanRows& R, const char* who) {
  if (!R.key || !R.count || !R.first || !R.last || !R.tmin || !R.tmax || !R.opens || !R.closes || !R.toklen || !R.tok)
    throw std::runtime_error(std::string(who) + ": missing row column");
  if (((uintptr_t)R.tok & 7) != 0) throw std::runtime_error(std::string(who) + ": the token column must be 8-byte aligned");
}

void span_fold_dev(const SpanTab& T, const SpanPairs& X, uint64_t stream) {
  st_check(T, "span_fold_dev");
  sp_check(X, "span_fold_dev");
  if (X.n <= 0) return;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const unsigned blocks = launch_blocks(X.n, 256, "span_fold_dev");
  hipLaunchKernelGGL(k_span_fold, dim3(blocks), dim3(256), 0, st, T, X);
  LP_HIP_CHECK(hipGetLastError());
}

void span_ends_dev(const SpanTab& T, const SpanPairs& X, uint64_t stream) {
  st_check(T, "span_ends_dev");
  sp_check(X, "span_ends_dev");
  if (X.n <= 0) return;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_span_ends, dim3(launch_blocks(X.n, 256, "span_ends_dev")), dim3(256), 0, st, T, X);
  LP_HIP_CHECK(hipGetLastError());
}

void span_rows_dev(const SpanTab& T, const SpanRows& R, int64_t out_cap, unsigned long long* cnt, uint64_t stream, int shift) {
  st_check(T, "span_rows_dev");
  if (shift < 0 || shift > 64) throw std::runtime_error("span_rows_dev: shift must be 0..64");
  if (out_cap > 0) sw_check(R, "span_rows_dev");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_span_rows, dim3(launch_blocks(T.cap + 1, SW_SLOTS, "span_rows_dev")), dim3(256), 0, st, T, R, out_cap, cnt,
                     shift);
  LP_HIP_CHECK(hipGetLastError());
}

void span_reinsert_dev(const SpanTab& T, const SpanRows& R, int64_t n, uint64_t stream) {
  st_check(T, "span_reinsert_dev");
  if (n <= 0) return;
  sw_check(R, "span_reinsert_dev");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_span_reinsert, dim3(launch_blocks(n, 256, "span_reinsert_dev")), dim3(256), 0, st, T, R, n);
  LP_HIP_CHECK(hipGetLastError());
}

// ---- host twins: the same table layout, one thread

static int64_t st_claim_host(const SpanTab& T, int64_t k) {
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

void span_fold_host(const SpanTab& T, const SpanPairs& X) {
  st_check(T, "span_fold_host");
  sp_check(X, "span_fold_host");
  for (int64_t i = 0; i < X.n; ++i) {
    const int64_t x = X.line[i];
    if (x < 0 || x >= X.nl) {
      ++T.used[1];
      continue;
    }
    const int64_t s = st_claim_host(T, X.key[i]);
    if (s < 0) continue;
    const long long g = X.line_base + x;
    ++T.count[s];
    T.first[s] = std::min<long long>(T.first[s], g);
    T.last[s] = std::max<long long>(T.last[s], g);
    const long long e = X.eff[x];
    if (e != TS_NONE) {
      T.tmin[s] = std::min<long long>(T.tmin[s], e);
      T.tmax[s] = std::max<long long>(T.tmax[s], e);
    }
  }
}

void span_ends_host(const SpanTab& T, const SpanPairs& X) {
  st_check(T, "span_ends_host");
  sp_check(X, "span_ends_host");
  for (int64_t i = 0; i < X.n; ++i) span_end_pair(T, X, i);
}

void span_rows_host(const SpanTab& T, const SpanRows& R, int64_t out_cap, unsigned long long* cnt, int shift) {
  st_check(T, "span_rows_host");
  if (shift < 0 || shift > 64) throw std::runtime_error("span_rows_host: shift must be 0..64");
  if (out_cap > 0) sw_check(R, "span_rows_host");
  unsigned long long o = *cnt;
  for (int64_t s = 0; s <= T.cap; ++s) {
    if (!st_listed(T, s, shift)) continue;
    if ((int64_t)o < out_cap) span_row_out(T, s, R, (int64_t)o);
    ++o;
  }
  *cnt = o;
}

void span_reinsert_host(const SpanTab& T, const SpanRows& R, int64_t n) {
  st_check(T, "span_reinsert_host");
  if (n > 0) sw_check(R, "span_reinsert_host");
  const unsigned long long used = T.used[0];      // (not counted here either: the caller writes it)
  for (int64_t i = 0; i < n; ++i) {
    const int64_t s = st_claim_host(T, R.key[i]);
    T.used[0] = used;
    if (s >= 0) span_row_in(T, s, R, i);
  }
}

}  // namespace lp
