// Log timeline: when did what happen? k_ts_parse reads the timestamp at the head of every line
// (ts_core.h line_ts_at); k_tl_hist counts lines, error lines, events and the events' severities
// per time bucket; between them k_tl_tiles / k_tl_prefix / k_tl_fill give unstamped lines the time of
// the nearest earlier stamped line and count the stamps that run backwards (two scans in line
// order). log_parser_amd/timeline.py drives them; log_parser_amd/golden.py timeline is the
// specification.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>
#include <string>

#include "gaps_core.h"
#include "lp_api.h"
#include "lp_block.h"
#include "lp_core.h"
#include "lp_host.h"
#include "ts_core.h"

namespace lp {

// one lane per line (k_gap_sig_list's form): a stamp at the head of the line settles within the
// lane's first two or three 16-byte loads
__global__ __launch_bounds__(256) void k_ts_parse(const uint8_t* __restrict__ text, int64_t tbytes,
                                                  const int64_t* __restrict__ ls, const int32_t* __restrict__ ll,
                                                  int64_t L, int64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= L) return;
  out[i] = line_ts_at(text, tbytes, ls[i], ll[i]);
}

void ts_parse_dev(const uint8_t* text, int64_t tbytes, const int64_t* ls, const int32_t* ll, int64_t L, int64_t* out,
                  uint64_t stream) {
  if (L <= 0) return;
  check_text_aligned(text, "ts_parse_dev");
  const unsigned blocks = launch_blocks(L, 256, "ts_parse_dev", "lines");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_ts_parse, dim3(blocks), dim3(256), 0, st, text, tbytes, ls, ll, L, out);
  LP_HIP_CHECK(hipGetLastError());
}

void ts_parse_host(const uint8_t* text, int64_t tbytes, const int64_t* ls, const int32_t* ll, int64_t L, int64_t* out) {
  if (L <= 0) return;
  host_parallel(L, 4096, [&](int, int64_t a, int64_t b) {
    for (int64_t i = a; i < b; ++i) out[i] = line_ts_at(text, tbytes, ls[i], ll[i]);
  });
}

// ---- forward fill and out-of-order count: two scans over the stamps in line order. `last` is the
// stamp of the nearest earlier stamped line (operator: the right operand unless it is TS_NONE),
// `top` the largest stamp so far (max; TS_NONE = INT64_MIN is its identity). Reduce-then-scan in
// three launches: k_tl_tiles (each tile's pair), k_tl_prefix (one block: the tiles' pairs become
// exclusive prefixes, the carries of earlier chunks first), k_tl_fill (scan inside the tile).
constexpr int TF_PER_LANE = 8;                       // consecutive lines of one lane
constexpr int TF_TILE = 256 * TF_PER_LANE;           // lines of one block

struct TfPair {
  int64_t last, top;
};

LP_HD TfPair tf_join(const TfPair& a, const TfPair& b) {
  return TfPair{b.last != TS_NONE ? b.last : a.last, a.top > b.top ? a.top : b.top};
}

// the pair of the lane's lines [i0, i0 + TF_PER_LANE) below L, and the stamps themselves
__device__ __forceinline__ TfPair tf_lane(const int64_t* __restrict__ ts, int64_t L, int64_t i0,
                                          int64_t (&v)[TF_PER_LANE]) {
  TfPair p{TS_NONE, TS_NONE};
#pragma unroll
  for (int j = 0; j < TF_PER_LANE; ++j) {
    v[j] = i0 + j < L ? ts[i0 + j] : TS_NONE;
    p = tf_join(p, TfPair{v[j], v[j]});
  }
  return p;
}

// the lane's EXCLUSIVE pair of the scan over the block, and the block's total in `total`
__device__ __forceinline__ TfPair tf_block_scan(TfPair mine, TfPair* s, TfPair& total) {
  return block_scan_excl(mine, TfPair{TS_NONE, TS_NONE}, s, total,
                         [](const TfPair& a, const TfPair& b) { return tf_join(a, b); });
}

__global__ __launch_bounds__(256) void k_tl_tiles(const int64_t* __restrict__ ts, int64_t L,
                                                  int64_t* __restrict__ t_last, int64_t* __restrict__ t_top) {
  __shared__ TfPair s[256];
  int64_t v[TF_PER_LANE];
  const int64_t i0 = (int64_t)blockIdx.x * TF_TILE + (int64_t)threadIdx.x * TF_PER_LANE;
  TfPair total;
  tf_block_scan(tf_lane(ts, L, i0, v), s, total);
  if (threadIdx.x == 0) {
    t_last[blockIdx.x] = total.last;
    t_top[blockIdx.x] = total.top;
  }
}

// one block: lane t owns the tiles [t * per, (t + 1) * per)
__global__ __launch_bounds__(256) void k_tl_prefix(int64_t* __restrict__ t_last, int64_t* __restrict__ t_top,
                                                   int64_t nt, int64_t carry_last, int64_t carry_top) {
  __shared__ TfPair s[256];
  const int64_t per = (nt + 255) / 256;
  const int64_t a = (int64_t)threadIdx.x * per, b = a + per < nt ? a + per : nt;
  TfPair p{TS_NONE, TS_NONE};
  for (int64_t k = a; k < b; ++k) p = tf_join(p, TfPair{t_last[k], t_top[k]});
  TfPair total;
  p = tf_join(TfPair{carry_last, carry_top}, tf_block_scan(p, s, total));
  for (int64_t k = a; k < b; ++k) {
    const TfPair own{t_last[k], t_top[k]};
    t_last[k] = p.last;
    t_top[k] = p.top;
    p = tf_join(p, own);
  }
}

__global__ __launch_bounds__(256) void k_tl_fill(const int64_t* __restrict__ ts, int64_t L,
                                                 const int64_t* __restrict__ t_last, const int64_t* __restrict__ t_top,
                                                 int64_t* __restrict__ eff, unsigned long long* __restrict__ ooo) {
  __shared__ TfPair s[256];
  __shared__ unsigned int s_ooo;
  if (threadIdx.x == 0) s_ooo = 0u;
  int64_t v[TF_PER_LANE];
  const int64_t i0 = (int64_t)blockIdx.x * TF_TILE + (int64_t)threadIdx.x * TF_PER_LANE;
  TfPair total;
  TfPair p = tf_block_scan(tf_lane(ts, L, i0, v), s, total);      // (its barriers order s_ooo = 0 as well)
  p = tf_join(TfPair{t_last[blockIdx.x], t_top[blockIdx.x]}, p);
  unsigned int n = 0u;
#pragma unroll
  for (int j = 0; j < TF_PER_LANE; ++j) {
    if (i0 + j >= L) break;
    n += (v[j] != TS_NONE && v[j] < p.top) ? 1u : 0u;
    p = tf_join(p, TfPair{v[j], v[j]});
    eff[i0 + j] = p.last;
  }
  if (n) atomicAdd(&s_ooo, n);
  __syncthreads();
  if (threadIdx.x == 0 && s_ooo) atomicAdd(ooo, (unsigned long long)s_ooo);
}

void tl_fill_dev(const int64_t* ts, int64_t L, int64_t carry_last, int64_t carry_top, int64_t* eff,
                 unsigned long long* ooo, int64_t* tmp, uint64_t stream) {
  if (L <= 0) return;
  const int64_t nt = launch_blocks(L, TF_TILE, "tl_fill_dev", "lines");
  if (!ts || !eff || !ooo || !tmp) throw std::runtime_error("tl_fill_dev: missing buffer");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  int64_t* t_last = tmp;
  int64_t* t_top = tmp + nt;
  hipLaunchKernelGGL(k_tl_tiles, dim3((unsigned)nt), dim3(256), 0, st, ts, L, t_last, t_top);
  LP_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_tl_prefix, dim3(1), dim3(256), 0, st, t_last, t_top, nt, carry_last, carry_top);
  LP_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_tl_fill, dim3((unsigned)nt), dim3(256), 0, st, ts, L, t_last, t_top, eff, ooo);
  LP_HIP_CHECK(hipGetLastError());
}

int64_t tl_fill_tmp_words(int64_t L) { return 2 * ((std::max<int64_t>(L, 0) + TF_TILE - 1) / TF_TILE); }

void tl_fill_host(const int64_t* ts, int64_t L, int64_t carry_last, int64_t carry_top, int64_t* eff,
                  unsigned long long* ooo) {
  TfPair p{carry_last, carry_top};
  unsigned long long n = 0;
  for (int64_t i = 0; i < L; ++i) {
    n += (ts[i] != TS_NONE && ts[i] < p.top) ? 1u : 0u;
    p = tf_join(p, TfPair{ts[i], ts[i]});
    eff[i] = p.last;
  }
  *ooo += n;
}

// ---- histogram. Item i < L is line i: columns 0 (lines) and 1 (error lines: gap_candidate of its
// features); item L + e is event e: columns 2 (events) and 3 + severity, in the bucket of its line.
// An item whose line is undated, or whose bucket lies outside [0, nb), is counted nowhere.
struct TlItem {
  int64_t bucket;   // -1: not counted
  int c0, c1;       // the two columns it counts in (c1 < 0: one column only)
};

LP_HD TlItem tl_item(const TlHistArgs& A, int64_t i) {
  TlItem it{-1, 0, -1};
  int64_t x = i;
  if (i >= A.L) {
    x = (int64_t)A.ev_line[i - A.L];
    if (x < 0 || x >= A.L) return it;
    const int64_t p = (int64_t)A.ev_pat[i - A.L];
    const int s = (p >= 0 && p < A.P) ? A.sev_index[p] : -1;
    it.c0 = 2;
    it.c1 = (s >= 0 && s < A.S) ? 3 + s : -1;
  } else {
    it.c1 = gap_candidate(A.feat[x]) ? 1 : -1;
  }
  const int64_t t = A.eff[x];
  if (t == TS_NONE || t < A.t0) return it;
  const int64_t b = (t - A.t0) / A.W;
  if (b < A.nb) it.bucket = b;
  return it;
}

// A log is roughly ordered by time, so the items of a tile land in a handful of buckets and global
// atomics would serialise on a few addresses: the block counts in an LDS table first (bucket ->
// one counter per column; k_gap_fold's scheme) and then issues one global atomic per (distinct
// bucket, non-zero counter). An item that finds no LDS slot within TL_LDS_PROBES probes -- more
// distinct buckets in the tile than the table takes -- goes to the global histogram directly.
constexpr int TL_TILE = 2048;            // items per block
constexpr int TL_LDS_SLOTS = 256;        // at most; fewer when 3 + S columns would not fit TL_LDS_BYTES
constexpr int TL_LDS_BYTES = 32768;
constexpr int TL_LDS_PROBES = 8;

__global__ __launch_bounds__(256) void k_tl_hist(TlHistArgs A, int slots) {
  extern __shared__ unsigned int tl_lds[];                   // [slots] keys, then [slots][C] counters
  using ull = unsigned long long;
  const int C = 3 + A.S;
  unsigned int* lkey = tl_lds;
  unsigned int* lcnt = tl_lds + slots;
  for (int j = threadIdx.x; j < slots * (C + 1); j += (int)blockDim.x) tl_lds[j] = j < slots ? 0xFFFFFFFFu : 0u;
  __syncthreads();
  const int64_t n = A.L + A.E;
  const int64_t base = (int64_t)blockIdx.x * TL_TILE;
  const int64_t end = base + TL_TILE < n ? base + TL_TILE : n;
  ull* hist = reinterpret_cast<ull*>(A.hist);
  for (int64_t i = base + threadIdx.x; i < end; i += blockDim.x) {
    const TlItem it = tl_item(A, i);
    if (it.bucket < 0) continue;
    const unsigned int key = (unsigned int)it.bucket;        // (nb < 2^31: checked by the launcher)
    int h = (int)(((key * 2654435761u) >> 16) & (unsigned int)(slots - 1));
    bool done = false;
    for (int p = 0; p < TL_LDS_PROBES && p < slots && !done; ++p) {
      const unsigned int v = atomicCAS(&lkey[h], 0xFFFFFFFFu, key);
      if (v == 0xFFFFFFFFu || v == key) {
        atomicAdd(&lcnt[h * C + it.c0], 1u);
        if (it.c1 >= 0) atomicAdd(&lcnt[h * C + it.c1], 1u);
        done = true;
      }
      h = (h + 1) & (slots - 1);
    }
    if (!done) {
      atomicAdd(hist + it.bucket * C + it.c0, 1ull);
      if (it.c1 >= 0) atomicAdd(hist + it.bucket * C + it.c1, 1ull);
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < slots * C; j += (int)blockDim.x) {
    const unsigned int v = lcnt[j];
    if (v) atomicAdd(hist + (int64_t)lkey[j / C] * C + j % C, (ull)v);   // (a counted slot has its key)
  }
}

static void tl_check(const TlHistArgs& A, const char* who) {
  if (A.L < 0 || A.E < 0 || A.S < 0 || A.P < 0) throw std::runtime_error(std::string(who) + ": negative size");
  if (A.W < 1) throw std::runtime_error(std::string(who) + ": bucket width must be positive");
  if (A.t0 <= -(1ll << 62) || A.t0 >= (1ll << 62)) throw std::runtime_error(std::string(who) + ": origin out of range");
  if (A.nb < 1 || A.nb > 0x7fffffffll) throw std::runtime_error(std::string(who) + ": bucket count out of range");
  if (!A.hist || (A.L && (!A.eff || !A.feat)) || (A.E && (!A.ev_line || !A.ev_pat || (A.P && !A.sev_index))))
    throw std::runtime_error(std::string(who) + ": missing input");
}

void tl_hist_dev(const TlHistArgs& A, uint64_t stream) {
  tl_check(A, "tl_hist_dev");
  const int64_t n = A.L + A.E;
  if (n <= 0) return;
  const int C = 3 + A.S;
  if ((int64_t)(C + 1) * 4 > TL_LDS_BYTES)
    throw std::runtime_error("tl_hist_dev: too many severities for the block table");
  int slots = TL_LDS_SLOTS;
  while ((int64_t)slots * (C + 1) * 4 > TL_LDS_BYTES) slots >>= 1;      // (a power of two, >= 1)
  const unsigned blocks = launch_blocks(n, TL_TILE, "tl_hist_dev");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_tl_hist, dim3(blocks), dim3(256), (size_t)slots * (C + 1) * 4, st, A, slots);
  LP_HIP_CHECK(hipGetLastError());
}

void tl_hist_host(const TlHistArgs& A) {
  tl_check(A, "tl_hist_host");
  const int C = 3 + A.S;
  for (int64_t i = 0; i < A.L + A.E; ++i) {
    const TlItem it = tl_item(A, i);
    if (it.bucket < 0) continue;
    ++A.hist[it.bucket * C + it.c0];
    if (it.c1 >= 0) ++A.hist[it.bucket * C + it.c1];
  }
}

}  // namespace lp
