// Correlation report: which lines of a log hold the ids that its event lines hold? k_line_keys walks
// lines (key_core.h line_keys_at) and writes their keys as compacted (line, key) pairs -- the first
// kernel here whose lines emit a VARIABLE number of records, 0..8. Two optional inputs make it
// serve both passes of log_parser_amd/correlate.py: `sel` walks a list of lines (pass 1: the event
// lines) and `tab`, a signature group table that is only read (gap_table.h), keeps the keys it
// holds (pass 2: every line, but only the event keys). The grouping of the pairs is the table work
// of gap_table.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

#include "gap_table.h"
#include "key_core.h"
#include "lp_api.h"
#include "lp_block.h"
#include "lp_core.h"
#include "lp_host.h"

namespace lp {

constexpr int KL_MAX_LINES = 2048;                  // lines per block at most
constexpr int KL_ROUND = 256;                       // lines per round: one per lane
constexpr int KL_STAGE = KL_ROUND * KEY_PER_LINE;   // pairs of a round at most: 24 KiB of LDS

// the line item i walks, or -1: none (past the end, or a `sel` entry that names no line)
__device__ __forceinline__ int64_t kl_line(const KeyLinesArgs& A, int64_t i) {
  if (i >= A.n) return -1;
  const int64_t x = A.sel ? (int64_t)A.sel[i] : i;
  return (x >= 0 && x < A.nl) ? x : -1;
}

// A block owns `per_block` consecutive items, one lane per line and round. A round's lanes hold
// 0..8 pairs each: an exclusive scan of the counts (block_excl_count) gives every lane its place in
// the round's LDS stage, the block reserves the round's output slots with ONE global atomic
// (block_reserve), and the stage is copied out coalesced.
__global__ __launch_bounds__(256) void k_line_keys(KeyLinesArgs A, int per_block) {
  __shared__ int64_t l_key[KL_STAGE];
  __shared__ int32_t l_line[KL_STAGE];
  __shared__ int s_wave[4];
  __shared__ int s_hit;
  __shared__ long long s_out;
  const int lane = threadIdx.x & 63;
  const bool filter = A.tab.key != nullptr;
  if (threadIdx.x == 0) s_hit = 0;
  const int64_t base = (int64_t)blockIdx.x * per_block;
  int hit_w = 0;                              // this wave's lines with a pair (every lane holds it)
  for (int k0 = 0; k0 < per_block; k0 += KL_ROUND) {          // uniform trip count: shuffles and barriers are whole-block
    const int64_t i = base + k0 + (int)threadIdx.x;           // (k0 + threadIdx.x < per_block: a multiple of 256)
    const int64_t x = kl_line(A, i);
    KeyList K;
    if (x >= 0) line_keys_at(A.text, A.tbytes, A.ls[x], A.ll[x], A.min_len, K);
    // the table's filter: bit j of `keep` -- slot j is emitted
    uint32_t keep = 0u;
#pragma unroll
    for (int j = 0; j < KEY_PER_LINE; ++j)
      if (j < K.n && (!filter || gt_find(A.tab, K.k[j]) >= 0)) keep |= 1u << j;
    const int c = __popc(keep);
    if (i < A.n) A.hit[i] = c ? 1 : 0;
    hit_w += __popcll(__ballot(c != 0));
    // exclusive scan of c over the round (its barrier also: the previous round's copy-out has read the stage)
    int total;
    int off = block_excl_count(c, s_wave, total);
    // stage: off + c <= total <= KL_STAGE
#pragma unroll
    for (int j = 0; j < KEY_PER_LINE; ++j) {
      if (keep & (1u << j)) {
        l_key[off] = K.k[j];
        l_line[off] = (int32_t)x;
        ++off;
      }
    }
    const int64_t o0 = block_reserve(A.cnt, total, &s_out);
    for (int j = threadIdx.x; j < total; j += KL_ROUND) {
      const int64_t o = o0 + j;
      if (o >= A.cap) break;                  // over capacity: counted above, the caller re-runs
      A.out_line[o] = l_line[j];
      A.out_key[o] = l_key[j];
    }
    // (the next round's scan barrier stands between this copy-out and its writes of the stage and
    // of s_out; its write of s_wave comes after block_reserve's barrier of this round)
  }
  if (lane == 0 && hit_w) atomicAdd(&s_hit, hit_w);
  __syncthreads();
  if (threadIdx.x == 0 && s_hit) atomicAdd(A.cnt + 1, (unsigned long long)s_hit);
}

static void kl_check(const KeyLinesArgs& A, const char* who) {
  const std::string w(who);
  if (A.min_len < KEY_MIN_LEN_LO || A.min_len > KEY_MAX_LEN)
    throw std::runtime_error(w + ": min_len must be " + std::to_string(KEY_MIN_LEN_LO) + ".." + std::to_string(KEY_MAX_LEN));
  if (A.nl < 0 || A.nl > 0x7fffffffll) throw std::runtime_error(w + ": too many lines for int32 line numbers");
  if (A.n < 0 || (!A.sel && A.n != A.nl)) throw std::runtime_error(w + ": without sel every line is walked");
  if (A.tab.key && (A.tab.cap < 1 || (A.tab.cap & (A.tab.cap - 1)) != 0))
    throw std::runtime_error(w + ": table capacity must be a power of two");
  if (A.cap < 0) throw std::runtime_error(w + ": negative capacity");
}

void line_keys_dev(const KeyLinesArgs& A, uint64_t stream, int per_block) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  kl_check(A, "line_keys_dev");
  check_text_aligned(A.text, "line_keys_dev");
  if (A.n <= 0) return;
  const LineGeom g = line_geom(A.n, per_block, KL_MAX_LINES, "line_keys_dev");
  hipLaunchKernelGGL(k_line_keys, dim3(g.blocks), dim3(256), 0, st, A, g.per);
  LP_HIP_CHECK(hipGetLastError());
}

void line_keys_host(const KeyLinesArgs& A) {
  kl_check(A, "line_keys_host");
  if (A.n <= 0) return;
  // every worker walks the items of its range; the ranges' pairs are appended in item order
  struct Row {
    int32_t line;
    int64_t key;
  };
  const int T = std::max(1, host_threads());
  std::vector<std::vector<Row>> part(T);
  std::vector<int64_t> hits(T, 0);
  host_parallel(A.n, 4096, [&](int t, int64_t a, int64_t b) {
    for (int64_t i = a; i < b; ++i) {
      const int64_t x = A.sel ? (int64_t)A.sel[i] : i;
      KeyList K;
      if (x >= 0 && x < A.nl) line_keys_at(A.text, A.tbytes, A.ls[x], A.ll[x], A.min_len, K);
      bool any = false;
      for (int j = 0; j < K.n; ++j) {
        if (A.tab.key && gt_find(A.tab, K.k[j]) < 0) continue;
        part[t].push_back({(int32_t)x, K.k[j]});
        any = true;
      }
      A.hit[i] = any ? 1 : 0;
      if (any) ++hits[t];
    }
  });
  int64_t o = 0, h = 0;
  for (int t = 0; t < T; ++t) {
    h += hits[t];
    for (const Row& r : part[t]) {
      if (o < A.cap) {
        A.out_line[o] = r.line;
        A.out_key[o] = r.key;
      }
      ++o;
    }
  }
  A.cnt[0] += (unsigned long long)o;
  A.cnt[1] += (unsigned long long)h;
}

}  // namespace lp
