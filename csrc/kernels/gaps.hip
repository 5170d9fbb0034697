// Coverage-gap report: which error lines of a log does no pattern of the library explain, grouped
// by shape? The matchers and the event stage have run; the context DFAs have classified every line
// (feat_all_dev). This file holds the one text kernel of the report: k_gap_sig picks the candidate
// lines (error keyword or exception class name, not a stack frame) that no event window covers and
// writes (line, template signature) pairs -- gaps_core.h line_sig_at. The grouping is integer tensor
// work on those pairs (engine.py gaps_bytes).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "gaps_core.h"
#include "lp_api.h"
#include "lp_block.h"
#include "lp_core.h"
#include "lp_host.h"

namespace lp {

// A block owns `per_block` consecutive lines (k_feat_cov's structure). Selected lines are a few
// percent of all lines and cost up to 1 KiB of dependent work each, so one lane per line would idle
// most of every wave: the block compacts its selected lines into an LDS list (wave_list_append) and
// its lanes then take lines from the list. The block reserves its output slots with ONE global
// atomic (block_reserve) -- the list's length is known before any line is signed.
constexpr int GS_MAX_LINES = 4096;   // lines per block (uint16 list entries)

__global__ __launch_bounds__(256) void k_gap_sig(GapSigArgs A, int per_block) {
  __shared__ uint16_t list[GS_MAX_LINES];   // block-relative numbers of the selected lines
  __shared__ int s_n, s_cand;
  __shared__ long long s_out;
  const int lane = threadIdx.x & 63;
  if (threadIdx.x == 0) {
    s_n = 0;
    s_cand = 0;
  }
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * per_block;
  int cand_w = 0;                            // this wave's candidates (every lane holds the count)
  for (int k0 = 0; k0 < per_block; k0 += (int)blockDim.x) {   // uniform trip count: ballots are whole-wave
    const int k = k0 + (int)threadIdx.x;
    const int64_t x = base + k;
    bool cand = false, pick = false;
    if (k < per_block && x < A.L) {
      cand = gap_candidate(A.feat[x]);
      pick = cand && !(A.cov && A.cov[x]);
    }
    cand_w += __popcll(__ballot(cand));
    const int j = wave_list_append(__ballot(pick), &s_n);
    if (pick) list[j] = (uint16_t)k;
  }
  if (lane == 0 && cand_w) atomicAdd(&s_cand, cand_w);
  __syncthreads();
  const int m = s_n;                         // <= per_block <= GS_MAX_LINES
  if (threadIdx.x == 0 && s_cand) atomicAdd(A.cnt, (unsigned long long)s_cand);
  const int64_t o0 = block_reserve(A.cnt + 1, m, &s_out);
  for (int j = threadIdx.x; j < m; j += (int)blockDim.x) {
    const int64_t o = o0 + j;
    if (o >= A.cap) break;                   // over capacity: counted above, the caller re-runs
    const int64_t x = base + list[j];
    A.out_line[o] = (int32_t)x;
    A.out_sig[o] = (int64_t)line_sig_at(A.text, A.tbytes, A.ls[x], A.ll[x]);
  }
}

// listed / every line: slot i signs line sel[i] (or line i). No selection, so one lane per slot.
__global__ __launch_bounds__(256) void k_gap_sig_list(GapSigArgs A, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = i < n;
  const unsigned long long m = __ballot(in);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(A.cnt + 1, (unsigned long long)__popcll(m));
  if (!in || i >= A.cap) return;
  const int64_t x = A.sel ? (int64_t)A.sel[i] : i;
  const bool ok = x >= 0 && x < A.L;
  A.out_line[i] = (int32_t)x;
  A.out_sig[i] = (int64_t)(ok ? line_sig_at(A.text, A.tbytes, A.ls[x], A.ll[x]) : SIG_FNV_OFFSET);
}

void gap_sig_dev(const GapSigArgs& A, uint64_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  check_text_aligned(A.text, "gap_sig_dev");
  if (A.sel || A.all) {
    const int64_t n = A.sel ? A.nsel : A.L;
    if (n <= 0) return;
    hipLaunchKernelGGL(k_gap_sig_list, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, A, n);
    LP_HIP_CHECK(hipGetLastError());
    return;
  }
  if (A.L <= 0) return;
  if (!A.feat) throw std::runtime_error("gap_sig_dev: the self-selecting form needs the features of every line");
  // lines per block: L / 1024 for a small document, 4096 for big ones
  const LineGeom g = line_geom(A.L, 0, GS_MAX_LINES, "gap_sig_dev", 1024);
  hipLaunchKernelGGL(k_gap_sig, dim3(g.blocks), dim3(256), 0, st, A, g.per);
  LP_HIP_CHECK(hipGetLastError());
}

void gap_sig_host(const GapSigArgs& A) {
  if (A.sel || A.all) {
    const int64_t n = A.sel ? A.nsel : A.L;
    host_parallel(std::min(n, A.cap), 1024, [&](int, int64_t a, int64_t b) {
      for (int64_t i = a; i < b; ++i) {
        const int64_t x = A.sel ? (int64_t)A.sel[i] : i;
        const bool ok = x >= 0 && x < A.L;
        A.out_line[i] = (int32_t)x;
        A.out_sig[i] = (int64_t)(ok ? line_sig_at(A.text, A.tbytes, A.ls[x], A.ll[x]) : SIG_FNV_OFFSET);
      }
    });
    A.cnt[1] += (unsigned long long)std::max<int64_t>(n, 0);
    return;
  }
  if (A.L <= 0) return;
  if (!A.feat) throw std::runtime_error("gap_sig_host: the self-selecting form needs the features of every line");
  // every worker signs the selected lines of its range; the ranges are appended in line order
  const int T = std::max(1, host_threads());
  std::vector<std::vector<std::pair<int32_t, int64_t>>> part(T);
  std::vector<int64_t> ncand(T, 0);
  host_parallel(A.L, 4096, [&](int t, int64_t a, int64_t b) {
    for (int64_t x = a; x < b; ++x) {
      if (!gap_candidate(A.feat[x])) continue;
      ++ncand[t];
      if (A.cov && A.cov[x]) continue;
      part[t].emplace_back((int32_t)x, (int64_t)line_sig_at(A.text, A.tbytes, A.ls[x], A.ll[x]));
    }
  });
  int64_t o = 0, nc = 0;
  for (int t = 0; t < T; ++t) {
    nc += ncand[t];
    for (const auto& pr : part[t]) {
      if (o < A.cap) {
        A.out_line[o] = pr.first;
        A.out_sig[o] = pr.second;
      }
      ++o;
    }
  }
  A.cnt[0] += (unsigned long long)nc;
  A.cnt[1] += (unsigned long long)o;
}

void feat_all_host(int64_t L, const uint8_t* text, const int64_t* ls, const int32_t* ll, const DfaPool& P,
                   uint8_t* feat) {
  if (L <= 0 || !feat) return;
  host_parallel(L, 4096, [&](int, int64_t a, int64_t b) {
    for (int64_t x = a; x < b; ++x) feat[x] = context_feat(P, text + ls[x], ll[x]);
  });
}

}  // namespace lp
