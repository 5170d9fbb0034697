// Values report: which numbers do the line templates of a log carry, and where do they peak?
// k_line_vals walks every line once (val_core.h line_vals_at: template signature and numeric
// fields in one pass), writes the signature of every line and the values as compacted
// (line, val_key(signature, field), value) triples -- 0..8 per line, on the block primitives of
// lp_block.h. The grouping of the triples is the table work of gap_table.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

#include "lp_api.h"
#include "lp_block.h"
#include "lp_core.h"
#include "lp_host.h"
#include "val_core.h"

namespace lp {

constexpr int VL_MAX_LINES = 2048;                  // lines per block at most
constexpr int VL_ROUND = 256;                       // lines per round: one per lane
constexpr int VL_STAGE = VL_ROUND * VAL_PER_LINE;   // triples of a round at most: 32 KiB of LDS

// A block owns `per_block` consecutive lines, one lane per line and round. A round's lanes hold
// 0..8 triples each: an exclusive scan of the counts (block_excl_count) gives every lane its place
// in the round's LDS stage, the block reserves the round's output slots with ONE global atomic
// (block_reserve), and the stage is copied out coalesced.
__global__ __launch_bounds__(256) void k_line_vals(ValLinesArgs A, int per_block) {
  __shared__ int64_t l_key[VL_STAGE];
  __shared__ int32_t l_line[VL_STAGE];
  __shared__ int32_t l_val[VL_STAGE];
  __shared__ int s_wave[4];
  __shared__ int s_hit;
  __shared__ long long s_out;
  const int lane = threadIdx.x & 63;
  if (threadIdx.x == 0) s_hit = 0;
  const int64_t base = (int64_t)blockIdx.x * per_block;
  int hit_w = 0;                              // this wave's lines with a value (every lane holds it)
  for (int k0 = 0; k0 < per_block; k0 += VL_ROUND) {          // uniform trip count: shuffles and barriers are whole-block
    const int64_t i = base + k0 + (int)threadIdx.x;           // (k0 + threadIdx.x < per_block: a multiple of 256)
    const bool live = i < A.nl;
    ValList V;
    uint64_t sig = 0;
    if (live) {
      sig = line_vals_at(A.text, A.tbytes, A.ls[i], A.ll[i], V);
      A.sig[i] = (int64_t)sig;
    }
    const int c = __popc(V.mask);
    hit_w += __popcll(__ballot(c != 0));
    // exclusive scan of c over the round (its barrier also: the previous round's copy-out has read the stage)
    int total;
    int off = block_excl_count(c, s_wave, total);
    // stage: off + c <= total <= VL_STAGE
#pragma unroll
    for (int j = 0; j < VAL_PER_LINE; ++j) {
      if (V.mask & (1u << j)) {
        l_key[off] = (int64_t)val_key(sig, j);
        l_line[off] = (int32_t)i;
        l_val[off] = V.v[j];
        ++off;
      }
    }
    const int64_t o0 = block_reserve(A.cnt, total, &s_out);
    for (int j = threadIdx.x; j < total; j += VL_ROUND) {
      const int64_t o = o0 + j;
      if (o >= A.cap) break;                  // over capacity: counted above, the caller re-runs
      A.out_line[o] = l_line[j];
      A.out_key[o] = l_key[j];
      A.out_val[o] = l_val[j];
    }
    // (the next round's scan barrier stands between this copy-out and its writes of the stage and
    // of s_out; its write of s_wave comes after block_reserve's barrier of this round)
  }
  if (lane == 0 && hit_w) atomicAdd(&s_hit, hit_w);
  __syncthreads();
  if (threadIdx.x == 0 && s_hit) atomicAdd(A.cnt + 1, (unsigned long long)s_hit);
}

static void vl_check(const ValLinesArgs& A, const char* who) {
  const std::string w(who);
  if (A.nl < 0 || A.nl > 0x7fffffffll) throw std::runtime_error(w + ": too many lines for int32 line numbers");
  if (A.tbytes < 0) throw std::runtime_error(w + ": negative text size");
  if (A.cap < 0) throw std::runtime_error(w + ": negative capacity");
}

void line_vals_dev(const ValLinesArgs& A, uint64_t stream, int per_block) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  vl_check(A, "line_vals_dev");
  check_text_aligned(A.text, "line_vals_dev");
  if (A.nl <= 0) return;
  const LineGeom g = line_geom(A.nl, per_block, VL_MAX_LINES, "line_vals_dev");
  hipLaunchKernelGGL(k_line_vals, dim3(g.blocks), dim3(256), 0, st, A, g.per);
  LP_HIP_CHECK(hipGetLastError());
}

void line_vals_host(const ValLinesArgs& A) {
  vl_check(A, "line_vals_host");
  if (A.nl <= 0) return;
  // every worker walks the lines of its range; the ranges' triples are appended in line order
  struct Row {
    int32_t line;
    int64_t key;
    int32_t val;
  };
  const int T = std::max(1, host_threads());
  std::vector<std::vector<Row>> part(T);
  std::vector<int64_t> hits(T, 0);
  host_parallel(A.nl, 4096, [&](int t, int64_t a, int64_t b) {
    for (int64_t i = a; i < b; ++i) {
      ValList V;
      const uint64_t sig = line_vals_at(A.text, A.tbytes, A.ls[i], A.ll[i], V);
      A.sig[i] = (int64_t)sig;
      for (int j = 0; j < VAL_PER_LINE; ++j)
        if (V.mask & (1u << j)) part[t].push_back({(int32_t)i, (int64_t)val_key(sig, j), V.v[j]});
      if (V.mask) ++hits[t];
    }
  });
  int64_t o = 0, h = 0;
  for (int t = 0; t < T; ++t) {
    h += hits[t];
    for (const Row& r : part[t]) {
      if (o < A.cap) {
        A.out_line[o] = r.line;
        A.out_key[o] = r.key;
        A.out_val[o] = r.val;
      }
      ++o;
    }
  }
  A.cnt[0] += (unsigned long long)o;
  A.cnt[1] += (unsigned long long)h;
}

}  // namespace lp
