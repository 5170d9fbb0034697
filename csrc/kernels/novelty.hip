// Novelty report: which lines of a log have a template that a baseline of healthy logs never
// showed? The baseline is a signature group table (gap_table.h) that this file only reads.
// k_novel_sig signs EVERY line (gaps_core.h line_sig_at), probes the table (gt_find) and writes the
// lines it does not find as (line, signature, flag) triples -- one read of the text, nothing
// written for the lines the baseline knows. k_gap_contains answers membership for a list of
// signatures. The grouping of the triples is the table work of gap_table.hip
// (log_parser_amd/novelty.py).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

#include "gap_table.h"
#include "gaps_core.h"
#include "lp_api.h"
#include "lp_block.h"
#include "lp_core.h"
#include "lp_host.h"

namespace lp {

// flag bits of a novel line
constexpr uint8_t NV_CAND = 1;    // gap_candidate(feat[x])
constexpr uint8_t NV_EVENT = 2;   // an event lies on the line

// A block owns `per_block` consecutive lines, one lane per line and round: every line is signed,
// so there is no selection to balance first. The novel lines of the block are compacted into an
// LDS list (wave_list_append: one LDS atomic per wave and round) WITH their signatures -- a
// signature costs up to 1 KiB of dependent work and is not computed twice -- and the block
// reserves its output slots with ONE global atomic (block_reserve) once the list is complete.
constexpr int NV_MAX_LINES = 2048;   // lines per block: 11 bytes of LDS each

__global__ __launch_bounds__(256) void k_novel_sig(NovelSigArgs A, int per_block) {
  __shared__ int64_t l_sig[NV_MAX_LINES];
  __shared__ uint16_t l_k[NV_MAX_LINES];      // block-relative numbers of the novel lines
  __shared__ uint8_t l_flag[NV_MAX_LINES];
  __shared__ int s_n, s_cand, s_ncand;
  __shared__ long long s_out;
  const int lane = threadIdx.x & 63;
  if (threadIdx.x == 0) {
    s_n = 0;
    s_cand = 0;
    s_ncand = 0;
  }
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * per_block;
  int cand_w = 0, ncand_w = 0;               // this wave's counts (every lane holds them)
  for (int k0 = 0; k0 < per_block; k0 += (int)blockDim.x) {   // uniform trip count: ballots are whole-wave
    const int k = k0 + (int)threadIdx.x;
    const int64_t x = base + k;
    bool cand = false, novel = false;
    uint8_t flag = 0;
    int64_t sig = 0;
    if (k < per_block && x < A.L) {
      cand = A.feat && gap_candidate(A.feat[x]);
      flag = (uint8_t)((cand ? NV_CAND : 0) | ((A.evm && A.evm[x]) ? NV_EVENT : 0));
      sig = (int64_t)line_sig_at(A.text, A.tbytes, A.ls[x], A.ll[x]);
      novel = gt_find(A.tab, sig) < 0;
    }
    const unsigned long long mc = __ballot(cand), mn = __ballot(novel);
    cand_w += __popcll(mc);
    ncand_w += __popcll(mc & mn);
    const int j = wave_list_append(mn, &s_n);   // < per_block <= NV_MAX_LINES
    if (novel) {
      l_sig[j] = sig;
      l_k[j] = (uint16_t)k;
      l_flag[j] = flag;
    }
  }
  if (lane == 0) {
    if (cand_w) atomicAdd(&s_cand, cand_w);
    if (ncand_w) atomicAdd(&s_ncand, ncand_w);
  }
  __syncthreads();
  const int m = s_n;                         // <= per_block <= NV_MAX_LINES
  if (threadIdx.x == 0) {
    if (s_cand) atomicAdd(A.cnt, (unsigned long long)s_cand);
    if (s_ncand) atomicAdd(A.cnt + 2, (unsigned long long)s_ncand);
  }
  const int64_t o0 = block_reserve(A.cnt + 1, m, &s_out);
  for (int j = threadIdx.x; j < m; j += (int)blockDim.x) {
    const int64_t o = o0 + j;
    if (o >= A.cap) break;                   // over capacity: counted above, the caller re-runs
    A.out_line[o] = (int32_t)(base + l_k[j]);
    A.out_sig[o] = l_sig[j];
    A.out_flag[o] = l_flag[j];
  }
}

// one lane per signature (the side slot of the empty marker is gt_find's business)
__global__ __launch_bounds__(256) void k_gap_contains(GapTab T, const int64_t* __restrict__ sig, int64_t n,
                                                      uint8_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = gt_find(T, sig[i]) >= 0 ? 1 : 0;
}

static void nv_check_tab(const GapTab& T, const char* who) {
  if (T.cap < 1 || (T.cap & (T.cap - 1)) != 0) throw std::runtime_error(std::string(who) + ": capacity must be a power of two");
  if (!T.key) throw std::runtime_error(std::string(who) + ": missing key column");
}

void novel_sig_dev(const NovelSigArgs& A, uint64_t stream, int per_block) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  nv_check_tab(A.tab, "novel_sig_dev");
  check_text_aligned(A.text, "novel_sig_dev");
  if (A.L <= 0) return;
  const LineGeom g = line_geom(A.L, per_block, NV_MAX_LINES, "novel_sig_dev");
  hipLaunchKernelGGL(k_novel_sig, dim3(g.blocks), dim3(256), 0, st, A, g.per);
  LP_HIP_CHECK(hipGetLastError());
}

void gap_contains_dev(const GapTab& T, const int64_t* sig, int64_t n, uint8_t* out, uint64_t stream) {
  nv_check_tab(T, "gap_contains_dev");
  if (n <= 0) return;
  const unsigned blocks = launch_blocks(n, 256, "gap_contains_dev", "signatures");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_gap_contains, dim3(blocks), dim3(256), 0, st, T, sig, n, out);
  LP_HIP_CHECK(hipGetLastError());
}

void novel_sig_host(const NovelSigArgs& A) {
  nv_check_tab(A.tab, "novel_sig_host");
  if (A.L <= 0) return;
  // every worker signs and probes the lines of its range; the ranges are appended in line order
  struct Row {
    int32_t line;
    uint8_t flag;
    int64_t sig;
  };
  const int T = std::max(1, host_threads());
  std::vector<std::vector<Row>> part(T);
  std::vector<int64_t> ncand(T, 0), nncand(T, 0);
  host_parallel(A.L, 4096, [&](int t, int64_t a, int64_t b) {
    for (int64_t x = a; x < b; ++x) {
      const bool cand = A.feat && gap_candidate(A.feat[x]);
      if (cand) ++ncand[t];
      const int64_t sig = (int64_t)line_sig_at(A.text, A.tbytes, A.ls[x], A.ll[x]);
      if (gt_find(A.tab, sig) >= 0) continue;
      if (cand) ++nncand[t];
      part[t].push_back({(int32_t)x, (uint8_t)((cand ? NV_CAND : 0) | ((A.evm && A.evm[x]) ? NV_EVENT : 0)), sig});
    }
  });
  int64_t o = 0, nc = 0, nnc = 0;
  for (int t = 0; t < T; ++t) {
    nc += ncand[t];
    nnc += nncand[t];
    for (const Row& r : part[t]) {
      if (o < A.cap) {
        A.out_line[o] = r.line;
        A.out_sig[o] = r.sig;
        A.out_flag[o] = r.flag;
      }
      ++o;
    }
  }
  A.cnt[0] += (unsigned long long)nc;
  A.cnt[1] += (unsigned long long)o;
  A.cnt[2] += (unsigned long long)nnc;
}

void gap_contains_host(const GapTab& T, const int64_t* sig, int64_t n, uint8_t* out) {
  nv_check_tab(T, "gap_contains_host");
  for (int64_t i = 0; i < n; ++i) out[i] = gt_find(T, sig[i]) >= 0 ? 1 : 0;
}

}  // namespace lp
