// Pauses report: where did a log go silent, and after which line templates? The input is what
// k_line_stamps gives per line (stamp, template signature); the stamped lines in line order are
// i_0 < i_1 < ..., the step k is ts[i_k] - ts[i_{k-1}] with the from-line i_{k-1} and the to-line
// i_k. A step below 0 is a backward step, a step >= min_ms a pause. Reduce-then-scan over the pair
// (stamp, line) of the last stamped line so far (operator: the right operand unless it has no
// stamp), 2,048 lines per block as the timeline's fill:
//
//   k_ps_tiles   per tile: its first stamp, its last stamped (stamp, line), its inner pauses
//   k_ps_prefix  one block: the tiles' pairs become exclusive prefixes (the carry of earlier runs
//                first), each tile's border step -- its first stamp against the incoming pair -- is
//                resolved, the pause counts become row offsets; the total and the new carry
//   k_ps_emit    scan inside the tile: every stamped line computes its step; interval histogram
//                and statistics per block, the pause rows at their offsets, in line order
//
// Rows, statistics and histogram are the host twin's on every run: the offsets come from counts,
// nothing is reserved with an atomic. log_parser_amd/pauses.py drives them;
// log_parser_amd/golden.py pauses is the specification.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>
#include <string>

#include "lp_api.h"
#include "lp_block.h"
#include "lp_core.h"
#include "lp_host.h"
#include "ts_core.h"

namespace lp {

namespace {
using ull = unsigned long long;
}

constexpr int PS_PER_LANE = 8;                       // consecutive lines of one lane
constexpr int PS_TILE = 256 * PS_PER_LANE;           // lines of one block

struct PsPair {
  int64_t ts, line;          // the last stamped line so far: its stamp (TS_NONE: none yet), its global number
};

LP_HD PsPair ps_join(const PsPair& a, const PsPair& b) { return b.ts != TS_NONE ? b : a; }

// to - from without signed overflow (the caller keeps stamps within +-2^61: no step wraps)
LP_HD int64_t ps_step(int64_t from, int64_t to) { return (int64_t)((uint64_t)to - (uint64_t)from); }

LP_HD bool ps_is_pause(int64_t step, int64_t min_ms) { return step >= min_ms; }     // (min_ms >= 1: never a backward step)

// bucket of a step >= 0: its bit length (0 for 0, b for [2^(b-1), 2^b)); at most 63
LP_HD int ps_bucket(int64_t step) { return step == 0 ? 0 : 64 - __builtin_clzll((ull)step); }

LP_HD int64_t ps_from_sig(const PauseArgs& A, int64_t from_line) {
  return from_line >= A.line_base ? A.sig[from_line - A.line_base] : A.carry_sig;
}

// the pair of the lane's lines [i0, i0 + PS_PER_LANE) below L, and the stamps themselves
__device__ __forceinline__ PsPair ps_lane(const int64_t* __restrict__ ts, int64_t L, int64_t line_base, int64_t i0,
                                          int64_t (&v)[PS_PER_LANE]) {
  PsPair p{TS_NONE, -1};
#pragma unroll
  for (int j = 0; j < PS_PER_LANE; ++j) {
    v[j] = i0 + j < L ? ts[i0 + j] : TS_NONE;
    p = ps_join(p, PsPair{v[j], line_base + i0 + j});
  }
  return p;
}

// the lane's EXCLUSIVE pair of the scan over the block, and the block's total in `total`
__device__ __forceinline__ PsPair ps_block_scan(PsPair mine, PsPair* s, PsPair& total) {
  return block_scan_excl(mine, PsPair{TS_NONE, -1}, s, total,
                         [](const PsPair& a, const PsPair& b) { return ps_join(a, b); });
}

__global__ __launch_bounds__(256) void k_ps_tiles(const int64_t* __restrict__ ts, int64_t L, int64_t line_base,
                                                  int64_t min_ms, int64_t* __restrict__ t_first,
                                                  int64_t* __restrict__ t_last, int64_t* __restrict__ t_line,
                                                  int64_t* __restrict__ t_cnt) {
  __shared__ PsPair s[256];
  __shared__ long long s_first;
  __shared__ unsigned int s_cnt;
  if (threadIdx.x == 0) {
    s_first = TS_NONE;
    s_cnt = 0u;
  }
  int64_t v[PS_PER_LANE];
  const int64_t i0 = (int64_t)blockIdx.x * PS_TILE + (int64_t)threadIdx.x * PS_PER_LANE;
  PsPair total;
  PsPair p = ps_block_scan(ps_lane(ts, L, line_base, i0, v), s, total);     // (its barriers order the two inits as well)
  unsigned int n = 0u;
#pragma unroll
  for (int j = 0; j < PS_PER_LANE; ++j) {
    if (v[j] == TS_NONE) continue;
    if (p.ts == TS_NONE) s_first = v[j];          // the tile's first stamped line: one writer
    else n += ps_is_pause(ps_step(p.ts, v[j]), min_ms) ? 1u : 0u;
    p = PsPair{v[j], 0};
  }
  n = wave_sum(n);
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(&s_cnt, n);
  __syncthreads();
  if (threadIdx.x == 0) {
    t_first[blockIdx.x] = s_first;
    t_last[blockIdx.x] = total.ts;
    t_line[blockIdx.x] = total.line;
    t_cnt[blockIdx.x] = (int64_t)s_cnt;
  }
}

// one block: lane t owns the tiles [t * per, (t + 1) * per). head: [0] the pauses of the run,
// [1..3] stamp, line and signature of the last stamped line so far (TS_NONE, -1, 0: none yet)
__global__ __launch_bounds__(256) void k_ps_prefix(PauseArgs A, int64_t* __restrict__ t_first,
                                                   int64_t* __restrict__ t_last, int64_t* __restrict__ t_line,
                                                   int64_t* __restrict__ t_cnt, int64_t nt) {
  __shared__ PsPair s[256];
  __shared__ long long s_sum[256];
  const int t = threadIdx.x;
  const int64_t per = (nt + 255) / 256;
  const int64_t a = (int64_t)t * per, b = a + per < nt ? a + per : nt;
  PsPair p{TS_NONE, -1};
  for (int64_t k = a; k < b; ++k) p = ps_join(p, PsPair{t_last[k], t_line[k]});
  const PsPair carry{A.carry_ts, A.carry_line};
  PsPair total;
  p = ps_join(carry, ps_block_scan(p, s, total));
  long long c = 0;
  for (int64_t k = a; k < b; ++k) {
    const PsPair own{t_last[k], t_line[k]};
    const int64_t f = t_first[k];
    // the border step: a tile without any stamp has none and passes the pair through
    const bool border = f != TS_NONE && p.ts != TS_NONE && ps_is_pause(ps_step(p.ts, f), A.min_ms);
    const long long n = t_cnt[k] + (border ? 1 : 0);
    t_cnt[k] = n;
    c += n;
    t_last[k] = p.ts;
    t_line[k] = p.line;
    p = ps_join(p, own);
  }
  long long sum;
  long long off = block_scan_excl(c, 0ll, s_sum, sum, [](long long x, long long y) { return x + y; });
  for (int64_t k = a; k < b; ++k) {
    const long long n = t_cnt[k];
    t_cnt[k] = off;
    off += n;
  }
  if (t == 255) {
    total = ps_join(carry, total);
    A.head[0] = sum;
    A.head[1] = total.ts;
    A.head[2] = total.ts != TS_NONE ? total.line : -1;
    A.head[3] = total.ts != TS_NONE ? ps_from_sig(A, total.line) : 0;
  }
}

__global__ __launch_bounds__(256) void k_ps_emit(PauseArgs A, const int64_t* __restrict__ t_last,
                                                 const int64_t* __restrict__ t_line,
                                                 const int64_t* __restrict__ t_off) {
  __shared__ PsPair s[256];
  __shared__ unsigned int s_hist[PS_BUCKETS];
  __shared__ int s_wave[4];
  __shared__ unsigned int s_stamped, s_back;
  __shared__ ull s_paused;
  __shared__ long long s_min, s_max;
  if (threadIdx.x < PS_BUCKETS) s_hist[threadIdx.x] = 0u;
  if (threadIdx.x == 0) {
    s_stamped = s_back = 0u;
    s_paused = 0ull;
    s_min = INT64_MAX;
    s_max = INT64_MIN;
  }
  int64_t v[PS_PER_LANE];
  const int64_t i0 = (int64_t)blockIdx.x * PS_TILE + (int64_t)threadIdx.x * PS_PER_LANE;
  PsPair total;
  PsPair p = ps_block_scan(ps_lane(A.ts, A.L, A.line_base, i0, v), s, total);   // (its barriers order the inits as well)
  p = ps_join(PsPair{t_last[blockIdx.x], t_line[blockIdx.x]}, p);
  // the lane's steps: counted here, the rows of its pauses written below
  unsigned int stamped = 0u, back = 0u;
  int c = 0;
  ull paused = 0ull;
  long long mn = INT64_MAX, mx = INT64_MIN;
  int hb = -1;                                    // neighbouring steps mostly share a bucket: one LDS atomic per run of them
  unsigned int hn = 0u;
  PsPair q = p;
#pragma unroll
  for (int j = 0; j < PS_PER_LANE; ++j) {
    if (v[j] == TS_NONE) continue;
    ++stamped;
    mn = v[j] < mn ? v[j] : mn;
    mx = v[j] > mx ? v[j] : mx;
    if (q.ts != TS_NONE) {
      const int64_t step = ps_step(q.ts, v[j]);
      if (step < 0) {
        ++back;
      } else {
        const int bk = ps_bucket(step);
        if (bk != hb) {
          if (hn) atomicAdd(&s_hist[hb], hn);
          hb = bk;
          hn = 0u;
        }
        ++hn;
        if (ps_is_pause(step, A.min_ms)) {
          ++c;
          paused += (ull)step;
        }
      }
    }
    q = PsPair{v[j], A.line_base + i0 + j};
  }
  if (hn) atomicAdd(&s_hist[hb], hn);
  // the statistics: per wave in registers, per block in LDS, then one set of global atomics
  stamped = wave_sum(stamped);
  back = wave_sum(back);
  paused = wave_reduce(paused, [](ull a, ull b) { return a + b; });
  mn = wave_reduce(mn, [](long long a, long long b) { return b < a ? b : a; });
  mx = wave_reduce(mx, [](long long a, long long b) { return b > a ? b : a; });
  if ((threadIdx.x & 63) == 0 && stamped) {
    atomicAdd(&s_stamped, stamped);
    if (back) atomicAdd(&s_back, back);
    if (paused) atomicAdd(&s_paused, paused);
    atomicMin(&s_min, mn);
    atomicMax(&s_max, mx);
  }
  // the lanes' places among the block's pause rows (the scan's barrier orders the LDS statistics too)
  int pauses;
  const int off = block_excl_count(c, s_wave, pauses);
  if (c) {
    int64_t o = t_off[blockIdx.x] + off;
    q = p;
#pragma unroll
    for (int j = 0; j < PS_PER_LANE; ++j) {
      if (v[j] == TS_NONE) continue;
      const int64_t to_line = A.line_base + i0 + j;
      if (q.ts != TS_NONE) {
        const int64_t step = ps_step(q.ts, v[j]);
        if (ps_is_pause(step, A.min_ms)) {
          if (o < A.cap) {                      // (the caller sizes the rows from the prefix pass's total)
            A.rows.to_line[o] = to_line;
            A.rows.from_line[o] = q.line;
            A.rows.ms[o] = step;
            A.rows.from_sig[o] = ps_from_sig(A, q.line);
            A.rows.to_sig[o] = A.sig[i0 + j];
          }
          ++o;
        }
      }
      q = PsPair{v[j], to_line};
    }
  }
  if (threadIdx.x < PS_BUCKETS && s_hist[threadIdx.x])
    atomicAdd(reinterpret_cast<ull*>(A.hist) + threadIdx.x, (ull)s_hist[threadIdx.x]);
  if (threadIdx.x == 0 && s_stamped) {
    ull* st = reinterpret_cast<ull*>(A.stats);
    atomicAdd(st + PS_STAMPED, (ull)s_stamped);
    if (s_back) atomicAdd(st + PS_BACKWARD, (ull)s_back);
    if (s_paused) atomicAdd(st + PS_PAUSED_MS, s_paused);
    atomicMin(reinterpret_cast<long long*>(A.stats) + PS_MIN_TS, s_min);
    atomicMax(reinterpret_cast<long long*>(A.stats) + PS_MAX_TS, s_max);
  }
}

static int64_t ps_tiles_of(int64_t L) { return (std::max<int64_t>(L, 0) + PS_TILE - 1) / PS_TILE; }

int64_t pause_tmp_words(int64_t L) { return 4 * ps_tiles_of(L); }

static void ps_check(const PauseArgs& A, bool emit, const char* who) {
  if (A.L < 0 || ps_tiles_of(A.L) > 0x7fffffffll) throw std::runtime_error(std::string(who) + ": too many lines for one launch");
  if (A.min_ms < 1) throw std::runtime_error(std::string(who) + ": min_ms must be at least 1");
  if (A.line_base < 0 || A.line_base > INT64_MAX - A.L) throw std::runtime_error(std::string(who) + ": line_base out of range");
  if (A.carry_ts != TS_NONE && (A.carry_line < 0 || A.carry_line >= A.line_base))
    throw std::runtime_error(std::string(who) + ": the carried line must lie before line_base");
  if (A.L && (!A.ts || !A.sig)) throw std::runtime_error(std::string(who) + ": missing input");
  if (!emit && !A.head) throw std::runtime_error(std::string(who) + ": missing head");
  if (emit) {
    if (!A.stats || !A.hist || A.cap < 0) throw std::runtime_error(std::string(who) + ": missing output");
    if (A.cap && (!A.rows.to_line || !A.rows.from_line || !A.rows.ms || !A.rows.from_sig || !A.rows.to_sig))
      throw std::runtime_error(std::string(who) + ": missing row column");
  }
}

void pause_count_dev(const PauseArgs& A, uint64_t stream) {
  ps_check(A, false, "pause_count_dev");
  if (A.L <= 0) return;
  if (!A.tmp) throw std::runtime_error("pause_count_dev: missing workspace");
  const int64_t nt = ps_tiles_of(A.L);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  int64_t *t_first = A.tmp, *t_last = A.tmp + nt, *t_line = A.tmp + 2 * nt, *t_cnt = A.tmp + 3 * nt;
  hipLaunchKernelGGL(k_ps_tiles, dim3((unsigned)nt), dim3(256), 0, st, A.ts, A.L, A.line_base, A.min_ms, t_first, t_last,
                     t_line, t_cnt);
  LP_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_ps_prefix, dim3(1), dim3(256), 0, st, A, t_first, t_last, t_line, t_cnt, nt);
  LP_HIP_CHECK(hipGetLastError());
}

void pause_emit_dev(const PauseArgs& A, uint64_t stream) {
  ps_check(A, true, "pause_emit_dev");
  if (A.L <= 0) return;
  if (!A.tmp) throw std::runtime_error("pause_emit_dev: missing workspace");
  const int64_t nt = ps_tiles_of(A.L);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_ps_emit, dim3((unsigned)nt), dim3(256), 0, st, A, A.tmp + nt, A.tmp + 2 * nt, A.tmp + 3 * nt);
  LP_HIP_CHECK(hipGetLastError());
}

// ---- host twins: one walk in line order

void pause_count_host(const PauseArgs& A) {
  ps_check(A, false, "pause_count_host");
  if (A.L <= 0) return;
  PsPair p{A.carry_ts, A.carry_line};
  int64_t n = 0;
  for (int64_t i = 0; i < A.L; ++i) {
    if (A.ts[i] == TS_NONE) continue;
    if (p.ts != TS_NONE && ps_is_pause(ps_step(p.ts, A.ts[i]), A.min_ms)) ++n;
    p = PsPair{A.ts[i], A.line_base + i};
  }
  A.head[0] = n;
  A.head[1] = p.ts;
  A.head[2] = p.ts != TS_NONE ? p.line : -1;
  A.head[3] = p.ts != TS_NONE ? ps_from_sig(A, p.line) : 0;
}

void pause_emit_host(const PauseArgs& A) {
  ps_check(A, true, "pause_emit_host");
  PsPair p{A.carry_ts, A.carry_line};
  int64_t o = 0;
  for (int64_t i = 0; i < A.L; ++i) {
    const int64_t t = A.ts[i];
    if (t == TS_NONE) continue;
    ++A.stats[PS_STAMPED];
    A.stats[PS_MIN_TS] = std::min(A.stats[PS_MIN_TS], t);
    A.stats[PS_MAX_TS] = std::max(A.stats[PS_MAX_TS], t);
    if (p.ts != TS_NONE) {
      const int64_t step = ps_step(p.ts, t);
      if (step < 0) {
        ++A.stats[PS_BACKWARD];
      } else {
        ++A.hist[ps_bucket(step)];
        if (ps_is_pause(step, A.min_ms)) {
          A.stats[PS_PAUSED_MS] = (int64_t)((uint64_t)A.stats[PS_PAUSED_MS] + (uint64_t)step);
          if (o < A.cap) {
            A.rows.to_line[o] = A.line_base + i;
            A.rows.from_line[o] = p.line;
            A.rows.ms[o] = step;
            A.rows.from_sig[o] = ps_from_sig(A, p.line);
            A.rows.to_sig[o] = A.sig[i];
          }
          ++o;
        }
      }
    }
    p = PsPair{t, A.line_base + i};
  }
}

}  // namespace lp
