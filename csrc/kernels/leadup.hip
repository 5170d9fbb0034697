// Lead-up report: which lines of a log lie within `W` lines before an event? k_lead_sig signs EVERY
// line (gaps_core.h line_sig_at), writes the signature of every line -- the report needs each
// template's total -- and marks the lines of the lead-up: x is in it iff some event line e of the
// sorted list `ev` has x < e <= x + W. The lead-up lines also come out as compacted (line,
// signature) pairs, so the fold of the few does not have to pick them out of the many. The grouping
// of both is the table work of gap_table.hip (log_parser_amd/leadup.py), and so is the carry
// between the pieces of a stream: this kernel knows the events of its own lines only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>
#include <string>

#include "gaps_core.h"
#include "lp_api.h"
#include "lp_block.h"
#include "lp_core.h"
#include "lp_host.h"

namespace lp {

constexpr int LD_MAX_LINES = 2048;   // lines per block: 10 bytes of LDS each
constexpr int LD_MAX_WINDOW = 4096;

// x is in the lead-up: the first event line after x (lower bound of x + 1 in the sorted, distinct
// ev[0, ne)) is at most W lines away. 64-bit: x + W must not wrap for a line near 2^31.
LP_HD bool lead_before_event(const int32_t* __restrict__ ev, int64_t ne, int64_t x, int W) {
  int64_t lo = 0, hi = ne;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if ((int64_t)ev[mid] < x + 1) lo = mid + 1;
    else hi = mid;
  }
  return lo < ne && (int64_t)ev[lo] <= x + (int64_t)W;
}

// A block owns `per_block` consecutive lines, one lane per line and round. The lead-up lines of the
// block are compacted into an LDS list (wave_list_append: one LDS atomic per wave and round) with
// their signatures, and the block reserves its output slots with ONE global atomic (block_reserve)
// once the list is complete.
__global__ __launch_bounds__(256) void k_lead_sig(LeadSigArgs A, int per_block) {
  __shared__ int64_t l_sig[LD_MAX_LINES];
  __shared__ uint16_t l_k[LD_MAX_LINES];      // block-relative numbers of the lead-up lines
  __shared__ int s_n;
  __shared__ long long s_out;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * per_block;
  for (int k0 = 0; k0 < per_block; k0 += (int)blockDim.x) {   // uniform trip count: ballots are whole-wave
    const int k = k0 + (int)threadIdx.x;
    const int64_t x = base + k;
    bool lead = false;
    int64_t sig = 0;
    if (k < per_block && x < A.L) {
      sig = (int64_t)line_sig_at(A.text, A.tbytes, A.ls[x], A.ll[x]);
      lead = lead_before_event(A.ev, A.ne, x, A.W);
      A.sig[x] = sig;
      A.lead[x] = lead ? 1 : 0;
    }
    const int j = wave_list_append(__ballot(lead), &s_n);   // < per_block <= LD_MAX_LINES
    if (lead) {
      l_sig[j] = sig;
      l_k[j] = (uint16_t)k;
    }
  }
  __syncthreads();
  const int m = s_n;                         // <= per_block <= LD_MAX_LINES
  const int64_t o0 = block_reserve(A.cnt, m, &s_out);
  for (int j = threadIdx.x; j < m; j += (int)blockDim.x) {
    const int64_t o = o0 + j;
    if (o >= A.cap) break;                   // over capacity: counted above, the caller re-runs
    A.out_line[o] = (int32_t)(base + l_k[j]);
    A.out_sig[o] = l_sig[j];
  }
}

static void ld_check(const LeadSigArgs& A, const char* who) {
  if (A.W < 1 || A.W > LD_MAX_WINDOW)
    throw std::runtime_error(std::string(who) + ": window must be 1.." + std::to_string(LD_MAX_WINDOW));
  if (A.ne < 0 || (A.ne > 0 && !A.ev)) throw std::runtime_error(std::string(who) + ": missing event lines");
  if (A.L > 0x7fffffffll) throw std::runtime_error(std::string(who) + ": too many lines for int32 line numbers");
}

void lead_sig_dev(const LeadSigArgs& A, uint64_t stream, int per_block) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  ld_check(A, "lead_sig_dev");
  check_text_aligned(A.text, "lead_sig_dev");
  if (A.L <= 0) return;
  const LineGeom g = line_geom(A.L, per_block, LD_MAX_LINES, "lead_sig_dev");
  hipLaunchKernelGGL(k_lead_sig, dim3(g.blocks), dim3(256), 0, st, A, g.per);
  LP_HIP_CHECK(hipGetLastError());
}

void lead_sig_host(const LeadSigArgs& A) {
  ld_check(A, "lead_sig_host");
  if (A.L <= 0) return;
  // every worker signs and marks the lines of its range; the ranges' pairs are appended in line order
  host_parallel(A.L, 4096, [&](int, int64_t a, int64_t b) {
    for (int64_t x = a; x < b; ++x) {
      A.sig[x] = (int64_t)line_sig_at(A.text, A.tbytes, A.ls[x], A.ll[x]);
      A.lead[x] = lead_before_event(A.ev, A.ne, x, A.W) ? 1 : 0;
    }
  });
  int64_t o = 0;
  for (int64_t x = 0; x < A.L; ++x) {
    if (!A.lead[x]) continue;
    if (o < A.cap) {
      A.out_line[o] = (int32_t)x;
      A.out_sig[o] = A.sig[x];
    }
    ++o;
  }
  A.cnt[0] += (unsigned long long)o;
}

}  // namespace lp
