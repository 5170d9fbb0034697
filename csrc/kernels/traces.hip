// Trace report: which stack traces does a log hold? k_tr_class classifies every line (trace_core.h
// trace_class_at) and computes what it contributes to a trace's signature -- the template
// signature of a frame (gaps_core.h line_sig_at, on FRAME lines only), the hash of a cause's
// token. The aggregate of every run of consecutive non-OTHER lines is a segmented inclusive scan
// in line order with the associative tr_combine: reduce-then-scan in three launches, k_tr_tiles
// (each tile's aggregate), k_tr_prefix (one block: the tiles' aggregates become exclusive
// prefixes), k_tr_emit (scan inside the tile; a line that ends a run with a frame writes one trace
// row). A run that came in from the previous piece of a stream is joined where it ends, in 64 bits
// (tr_close), and the run that is open at the end of the piece goes out the same way.
// log_parser_amd/traces.py drives them; log_parser_amd/golden.py traces is the specification.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>
#include <string>

#include "lp_api.h"
#include "lp_block.h"
#include "lp_core.h"
#include "lp_host.h"
#include "trace_core.h"

namespace lp {

constexpr int TR_PER_LANE = 4;                       // consecutive lines of one lane
constexpr int TR_TILE_LINES = 256 * TR_PER_LANE;     // lines of one block

int trace_tile() { return TR_TILE_LINES; }

// one lane per line
__global__ __launch_bounds__(256) void k_tr_class(const uint8_t* __restrict__ text, int64_t tbytes,
                                                  const int64_t* __restrict__ ls, const int32_t* __restrict__ ll,
                                                  int64_t L, uint8_t* __restrict__ cls, uint64_t* __restrict__ elem) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= L) return;
  uint8_t c;
  elem[i] = trace_element(text, tbytes, ls[i], ll[i], &c);
  cls[i] = c;
}

// the aggregate of the lane's lines [i0, i0 + TR_PER_LANE) below L
__device__ __forceinline__ TrAgg tr_lane(const TraceRunArgs& A, int64_t i0) {
  TrAgg p = tr_identity();
#pragma unroll
  for (int j = 0; j < TR_PER_LANE; ++j) {
    const int64_t i = i0 + j;
    if (i < A.L) p = tr_combine(p, tr_line(A.cls[i], A.elem[i], A.evm && A.evm[i], (int32_t)i));
  }
  return p;
}

// the lane's EXCLUSIVE aggregate of the scan over the block, and the block's total in `total`
__device__ __forceinline__ TrAgg tr_block_scan(const TrAgg& mine, TrAgg* s, TrAgg& total) {
  return block_scan_excl(mine, tr_identity(), s, total,
                         [](const TrAgg& a, const TrAgg& b) { return tr_combine(a, b); });
}

__global__ __launch_bounds__(256) void k_tr_tiles(TraceRunArgs A, TrAgg* __restrict__ tiles) {
  __shared__ TrAgg s[256];
  const int64_t i0 = (int64_t)blockIdx.x * TR_TILE_LINES + (int64_t)threadIdx.x * TR_PER_LANE;
  TrAgg total;
  tr_block_scan(tr_lane(A, i0), s, total);
  if (threadIdx.x == 0) tiles[blockIdx.x] = total;
}

// one block: lane t owns the tiles [t * per, (t + 1) * per)
__global__ __launch_bounds__(256) void k_tr_prefix(TrAgg* __restrict__ tiles, int64_t nt) {
  __shared__ TrAgg s[256];
  const int64_t per = (nt + 255) / 256;
  const int64_t a = (int64_t)threadIdx.x * per, b = a + per < nt ? a + per : nt;
  TrAgg p = tr_identity();
  for (int64_t k = a; k < b; ++k) p = tr_combine(p, tiles[k]);
  TrAgg total;
  p = tr_block_scan(p, s, total);
  for (int64_t k = a; k < b; ++k) {
    const TrAgg own = tiles[k];
    tiles[k] = p;
    p = tr_combine(p, own);
  }
}

__device__ __forceinline__ void tr_store_carry(int64_t* __restrict__ out, const TrCarry& c) {
  out[0] = c.open;
  out[1] = (int64_t)c.pow;
  out[2] = (int64_t)c.val;
  out[3] = c.frames;
  out[4] = c.causes;
  out[5] = c.lines;
  out[6] = c.event;
  out[7] = c.headless;
  out[8] = c.start;
  out[9] = c.ff;
  out[10] = c.lc;
  out[11] = c.prev_event;
  out[12] = c.has_prev;
}

__device__ __forceinline__ void tr_put(const TraceRunArgs& A, int64_t o, const TrRow& r) {
  if (o >= A.cap) return;                            // over capacity: counted, the caller re-runs
  int64_t* out = A.out;
  out[0 * A.cap + o] = r.start;
  out[1 * A.cap + o] = r.sig;
  out[2 * A.cap + o] = r.lines;
  out[3 * A.cap + o] = r.frames;
  out[4 * A.cap + o] = r.causes;
  out[5 * A.cap + o] = r.flags;
  out[6 * A.cap + o] = r.ff;
  out[7 * A.cap + o] = r.lc;
}

// The lane's lines [i0, i0 + TR_PER_LANE) below L, p the aggregate of the piece's lines before
// them: returns the number of rows they give. WRITE: the rows go to the slots from `o` on, and the
// lane of the last line writes the carry out.
template <bool WRITE>
__device__ __forceinline__ unsigned tr_walk(const TraceRunArgs& A, TrAgg p, int64_t i0, int64_t o) {
  unsigned n = 0;
  // the run that came in and ended with the previous piece: line 0 is OTHER
  if (i0 == 0 && A.L > 0 && A.in.open && A.in.frames > 0 && A.cls[0] == TR_OTHER) {
    if (WRITE) tr_put(A, o, tr_row(A.in));
    ++n;
  }
#pragma unroll
  for (int j = 0; j < TR_PER_LANE; ++j) {
    const int64_t i = i0 + j;
    if (i >= A.L) break;
    const uint8_t c = A.cls[i];
    p = tr_combine(p, tr_line(c, A.elem[i], A.evm && A.evm[i], (int32_t)i));
    const bool tail = i + 1 == A.L;
    if (c != TR_OTHER && (tail ? A.last : A.cls[i + 1] == TR_OTHER)) {
      const TrCarry run = tr_close(p, i, A.in, A.evm, 0);
      if (run.frames > 0) {
        if (WRITE) tr_put(A, o + n, tr_row(run));
        ++n;
      }
    }
    if (WRITE && tail) {
      const bool ev = A.evm && A.evm[i];
      tr_store_carry(A.carry_out, (c != TR_OTHER && !A.last) ? tr_close(p, i, A.in, A.evm, A.L) : tr_no_carry(ev));
    }
  }
  return n;
}

// The lanes count their rows first; the block reserves its output slots with ONE global atomic
// (block_reserve: thousands of returning atomics on one address would serialise), and the lanes
// walk their lines a second time to write.
__global__ __launch_bounds__(256) void k_tr_emit(TraceRunArgs A, const TrAgg* __restrict__ tiles) {
  __shared__ TrAgg s[256];
  __shared__ unsigned int s_n;
  __shared__ long long s_base;
  if (threadIdx.x == 0) s_n = 0u;
  const int64_t i0 = (int64_t)blockIdx.x * TR_TILE_LINES + (int64_t)threadIdx.x * TR_PER_LANE;
  TrAgg total;
  TrAgg p = tr_block_scan(tr_lane(A, i0), s, total);   // (its barriers order s_n = 0 as well)
  p = tr_combine(tiles[blockIdx.x], p);
  const unsigned mine = tr_walk<false>(A, p, i0, 0);
  const unsigned at = mine ? atomicAdd(&s_n, mine) : 0u;
  __syncthreads();
  tr_walk<true>(A, p, i0, block_reserve(A.cnt, (int)s_n, &s_base) + at);
}

static void tr_check(const TraceRunArgs& A, const char* who) {
  if (A.L <= 0) throw std::runtime_error(std::string(who) + ": no lines");
  if (A.L > 0x7fffffffll) throw std::runtime_error(std::string(who) + ": too many lines for one piece");
  if (!A.cls || !A.elem || !A.out || !A.cnt || !A.carry_out) throw std::runtime_error(std::string(who) + ": missing buffer");
  if (A.cap < 1) throw std::runtime_error(std::string(who) + ": capacity must be positive");
}

void trace_class_dev(const uint8_t* text, int64_t tbytes, const int64_t* ls, const int32_t* ll, int64_t L, uint8_t* cls,
                     uint64_t* elem, uint64_t stream) {
  if (L <= 0) return;
  check_text_aligned(text, "trace_class_dev");
  const unsigned blocks = launch_blocks(L, 256, "trace_class_dev", "lines");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_tr_class, dim3(blocks), dim3(256), 0, st, text, tbytes, ls, ll, L, cls, elem);
  LP_HIP_CHECK(hipGetLastError());
}

void trace_class_host(const uint8_t* text, int64_t tbytes, const int64_t* ls, const int32_t* ll, int64_t L, uint8_t* cls,
                      uint64_t* elem) {
  if (L <= 0) return;
  host_parallel(L, 4096, [&](int, int64_t a, int64_t b) {
    for (int64_t i = a; i < b; ++i) elem[i] = trace_element(text, tbytes, ls[i], ll[i], &cls[i]);
  });
}

int64_t trace_runs_tmp_bytes(int64_t L) {
  return (int64_t)sizeof(TrAgg) * ((std::max<int64_t>(L, 0) + TR_TILE_LINES - 1) / TR_TILE_LINES);
}

void trace_runs_dev(const TraceRunArgs& A, void* tmp, uint64_t stream) {
  tr_check(A, "trace_runs_dev");
  if (!tmp || ((uintptr_t)tmp & 7) != 0) throw std::runtime_error("trace_runs_dev: missing or misaligned scratch buffer");
  const int64_t nt = (A.L + TR_TILE_LINES - 1) / TR_TILE_LINES;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  TrAgg* tiles = reinterpret_cast<TrAgg*>(tmp);
  hipLaunchKernelGGL(k_tr_tiles, dim3((unsigned)nt), dim3(256), 0, st, A, tiles);
  LP_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_tr_prefix, dim3(1), dim3(256), 0, st, tiles, nt);
  LP_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_tr_emit, dim3((unsigned)nt), dim3(256), 0, st, A, (const TrAgg*)tiles);
  LP_HIP_CHECK(hipGetLastError());
}

// the same rows in line order, by the same combine one line at a time
void trace_runs_host(const TraceRunArgs& A) {
  tr_check(A, "trace_runs_host");
  int64_t n = 0;
  auto put = [&](const TrRow& r) {
    if (n < A.cap) {
      const int64_t v[TR_COLS] = {r.start, r.sig, r.lines, r.frames, r.causes, r.flags, r.ff, r.lc};
      for (int c = 0; c < TR_COLS; ++c) A.out[c * A.cap + n] = v[c];
    }
    ++n;
  };
  if (A.in.open && A.in.frames > 0 && A.cls[0] == TR_OTHER) put(tr_row(A.in));
  TrAgg p = tr_identity();
  TrCarry co = tr_no_carry(false);
  for (int64_t i = 0; i < A.L; ++i) {
    const uint8_t c = A.cls[i];
    p = tr_combine(p, tr_line(c, A.elem[i], A.evm && A.evm[i], (int32_t)i));
    const bool tail = i + 1 == A.L;
    if (c != TR_OTHER && (tail ? A.last : A.cls[i + 1] == TR_OTHER)) {
      const TrCarry run = tr_close(p, i, A.in, A.evm, 0);
      if (run.frames > 0) put(tr_row(run));
    }
    if (tail) co = (c != TR_OTHER && !A.last) ? tr_close(p, i, A.in, A.evm, A.L) : tr_no_carry(A.evm && A.evm[i]);
  }
  const int64_t w[TR_CARRY_WORDS] = {co.open, (int64_t)co.pow, (int64_t)co.val, co.frames, co.causes, co.lines, co.event,
                                     co.headless, co.start, co.ff, co.lc, co.prev_event, co.has_prev};
  for (int k = 0; k < TR_CARRY_WORDS; ++k) A.carry_out[k] = w[k];
  A.cnt[0] += (unsigned long long)n;
}

}  // namespace lp
