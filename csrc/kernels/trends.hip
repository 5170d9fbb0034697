// Trends report: which line templates of a log started, stopped or surged over its time?
// k_line_stamps walks every line once for its stamp and its template signature (ts_core.h
// line_ts_at, gaps_core.h line_sig_at); the cell table (cell_table.h) counts the lines per
// (signature, time bucket) across launches:
//
//   k_cell_fold      (signature, effective time) of consecutive lines -> table
//   k_cell_rows      occupied slots -> rows (sig, bucket, count, first)
//   k_cell_reinsert  rows of distinct cells -> a fresh table (growth)
//
// log_parser_amd/trends.py drives them; log_parser_amd/golden.py trends is the specification.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>
#include <string>

#include "cell_table.h"
#include "gaps_core.h"
#include "lp_api.h"
#include "lp_block.h"
#include "lp_core.h"
#include "lp_host.h"
#include "ts_core.h"

namespace lp {

namespace {
using ull = unsigned long long;
}

constexpr int LS_MAX_LINES = 2048;   // lines per block at most

// A block owns `per_block` consecutive lines (line_geom), one lane per line and round; nothing is
// compacted. The stamp comes first: its walk ends within the line's first 67 bytes, and
// the signature walk then finds the head of the line in cache.
__global__ __launch_bounds__(256) void k_line_stamps(LineStampsArgs A, int per_block) {
  const int64_t base = (int64_t)blockIdx.x * per_block;
  for (int k0 = 0; k0 < per_block; k0 += 256) {
    const int64_t i = base + k0 + (int)threadIdx.x;           // (k0 + threadIdx.x < per_block: a multiple of 256)
    if (i >= A.nl) break;
    const int64_t s = A.ls[i];
    const int n = A.ll[i];
    A.ts[i] = line_ts_at(A.text, A.tbytes, s, n);
    A.sig[i] = (int64_t)line_sig_at(A.text, A.tbytes, s, n);
  }
}

static void ls_check(const LineStampsArgs& A, const char* who) {
  if (A.nl < 0 || A.nl > 0x7fffffffll) throw std::runtime_error(std::string(who) + ": too many lines for one launch");
  if (A.tbytes < 0) throw std::runtime_error(std::string(who) + ": negative text size");
}

void line_stamps_dev(const LineStampsArgs& A, uint64_t stream, int per_block) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  ls_check(A, "line_stamps_dev");
  check_text_aligned(A.text, "line_stamps_dev");
  if (A.nl <= 0) return;
  const LineGeom g = line_geom(A.nl, per_block, LS_MAX_LINES, "line_stamps_dev");
  hipLaunchKernelGGL(k_line_stamps, dim3(g.blocks), dim3(256), 0, st, A, g.per);
  LP_HIP_CHECK(hipGetLastError());
}

void line_stamps_host(const LineStampsArgs& A) {
  ls_check(A, "line_stamps_host");
  if (A.nl <= 0) return;
  host_parallel(A.nl, 4096, [&](int, int64_t a, int64_t b) {
    for (int64_t i = a; i < b; ++i) {
      A.ts[i] = line_ts_at(A.text, A.tbytes, A.ls[i], A.ll[i]);
      A.sig[i] = (int64_t)line_sig_at(A.text, A.tbytes, A.ls[i], A.ll[i]);
    }
  });
}

// ---- the cell table

namespace {

// `cnt` lines of the cell (sig, bucket), the smallest of them `line`, into slot s, the slot that
// gt_claim (gap_table.h) gave for cell_key(sig, bucket). Everyone who flushes into a slot writes
// the same signature and bucket: plain stores.
__device__ __forceinline__ void ct_apply(const CellTab& T, int64_t s, int64_t sig, int64_t bucket, ull cnt,
                                         long long line) {
  T.sig[s] = sig;
  T.bucket[s] = bucket;
  atomicAdd(T.count + s, cnt);
  atomicMin(T.first + s, line);
}

}  // namespace

// A block owns `tile` consecutive lines (256..CT_TILE). Neighbouring lines mostly share a bucket and
// a few templates make most of a log, so the tile has few distinct cells: the block groups it in an
// LDS table (k_gap_fold's scheme: CAS on the key, bounded probes, LDS atomics for count and
// smallest line) and then issues one set of global atomics per distinct cell. A line that finds no
// LDS slot within CT_LDS_PROBES probes and the cell whose key equals the empty marker go to the
// global table directly. Bucket and key live in registers only.
constexpr int CT_TILE = 2048;
constexpr int CT_BLOCKS = 512;
constexpr int CT_LDS_SLOTS = 1024;
constexpr int CT_LDS_PROBES = 8;

__global__ __launch_bounds__(256) void k_cell_fold(CellTab T, const int64_t* __restrict__ sig,
                                                   const int64_t* __restrict__ eff, int64_t n, int64_t line_base,
                                                   int64_t W, int tile) {
  __shared__ ull lkey[CT_LDS_SLOTS];
  __shared__ long long lsig[CT_LDS_SLOTS];
  __shared__ long long lbkt[CT_LDS_SLOTS];
  __shared__ long long lmin[CT_LDS_SLOTS];
  __shared__ unsigned int lcnt[CT_LDS_SLOTS];
  __shared__ unsigned int s_fresh;
  if (threadIdx.x == 0) s_fresh = 0u;
  for (int j = threadIdx.x; j < CT_LDS_SLOTS; j += (int)blockDim.x) {
    lkey[j] = (ull)GT_EMPTY;
    lmin[j] = INT64_MAX;
    lcnt[j] = 0u;
  }
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * tile;
  const int64_t end = base + tile < n ? base + tile : n;
  for (int64_t i = base + threadIdx.x; i < end; i += blockDim.x) {
    const int64_t s = sig[i];
    const int64_t b = cell_bucket(eff[i], W);
    const int64_t k = cell_key(s, b);
    const long long g = line_base + i;
    bool done = false;
    if (k != GT_EMPTY) {
      int h = (int)((gt_hash(k) >> 40) & (uint64_t)(CT_LDS_SLOTS - 1));   // (not the bits of the global slot)
      for (int p = 0; p < CT_LDS_PROBES && !done; ++p) {
        const ull v = atomicCAS(&lkey[h], (ull)GT_EMPTY, (ull)k);
        if (v == (ull)GT_EMPTY || v == (ull)k) {
          lsig[h] = s;                        // (the same values from every line of the cell)
          lbkt[h] = b;
          atomicAdd(&lcnt[h], 1u);
          atomicMin(&lmin[h], g);
          done = true;
        }
        h = (h + 1) & (CT_LDS_SLOTS - 1);
      }
    }
    if (!done) {
      const int64_t t = gt_claim(T, k, &s_fresh);
      if (t >= 0) ct_apply(T, t, s, b, 1ull, g);
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < CT_LDS_SLOTS; j += (int)blockDim.x) {
    const ull k = lkey[j];
    if (k == (ull)GT_EMPTY) continue;
    const int64_t t = gt_claim(T, (int64_t)k, &s_fresh);
    if (t >= 0) ct_apply(T, t, lsig[j], lbkt[j], (ull)lcnt[j], lmin[j]);
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_fresh) atomicAdd(T.used, (ull)s_fresh);
}

// A block owns CR_SLOTS consecutive slots (the side slot included), a lane CR_ROUNDS of them. The
// block reserves its output rows with ONE global atomic: a table sized for the lines folded has
// millions of slots, and a reservation per wave (k_gap_rows) puts tens of thousands of atomics on
// one address -- they, not the slots' bytes, were the kernel's time.
constexpr int CR_ROUNDS = 8;
constexpr int CR_SLOTS = 256 * CR_ROUNDS;

__global__ __launch_bounds__(256) void k_cell_rows(CellTab T, CellRows R, int64_t out_cap, ull* cnt) {
  __shared__ int s_wave[4];
  __shared__ long long s_out;
  const int64_t base = (int64_t)blockIdx.x * CR_SLOTS + (int)threadIdx.x;
  unsigned int occ = 0u;                      // bit r: slot base + 256 r is occupied
#pragma unroll
  for (int r = 0; r < CR_ROUNDS; ++r) {
    const int64_t s = base + 256 * r;
    if (s <= T.cap && ct_occupied(T, s)) occ |= 1u << r;
  }
  int total;
  const int off = block_excl_count(__popc(occ), s_wave, total);
  int64_t o = block_reserve(cnt, total, &s_out) + off;
#pragma unroll
  for (int r = 0; r < CR_ROUNDS; ++r) {
    if (!(occ & (1u << r))) continue;
    const int64_t s = base + 256 * r;
    if (o < out_cap) {                       // over capacity: counted, the caller sees cnt > out_cap
      R.sig[o] = T.sig[s];
      R.bucket[o] = T.bucket[s];
      R.count[o] = (int64_t)T.count[s];
      R.first[o] = T.first[s];
    }
    ++o;
  }
}

// rows of DISTINCT cells into a table that holds none of them: the claim is the only atomic
// (used[0] is not counted here: it is n, and the caller writes it)
__global__ __launch_bounds__(256) void k_cell_reinsert(CellTab T, CellRows R, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t t = gt_claim(T, cell_key(R.sig[i], R.bucket[i]), nullptr);
  if (t < 0) return;
  T.sig[t] = R.sig[i];
  T.bucket[t] = R.bucket[i];
  T.count[t] = (ull)R.count[i];
  T.first[t] = R.first[i];
}

static void ct_check(const CellTab& T, const char* who) {
  if (T.cap < 1 || (T.cap & (T.cap - 1)) != 0) throw std::runtime_error(std::string(who) + ": capacity must be a power of two");
  if (!T.key || !T.sig || !T.bucket || !T.count || !T.first || !T.used)
    throw std::runtime_error(std::string(who) + ": missing table column");
}

static void cr_check(const CellRows& R, const char* who) {
  if (!R.sig || !R.bucket || !R.count || !R.first) throw std::runtime_error(std::string(who) + ": missing row column");
}

void cell_fold_dev(const CellTab& T, const int64_t* sig, const int64_t* eff, int64_t n, int64_t line_base, int64_t W,
                   uint64_t stream, int tile) {
  ct_check(T, "cell_fold_dev");
  if (W < 1) throw std::runtime_error("cell_fold_dev: the bucket width must be at least 1");
  if (n <= 0) return;
  if (tile <= 0) tile = (int)std::min<int64_t>(CT_TILE, std::max<int64_t>(256, (n / CT_BLOCKS + 255) / 256 * 256));
  if (tile < 256 || tile > CT_TILE || tile % 256) throw std::runtime_error("cell_fold_dev: tile must be 256..2048, a multiple of 256");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_cell_fold, dim3(launch_blocks(n, tile, "cell_fold_dev")), dim3(256), 0, st, T, sig, eff, n, line_base,
                     W, tile);
  LP_HIP_CHECK(hipGetLastError());
}

void cell_rows_dev(const CellTab& T, const CellRows& R, int64_t out_cap, unsigned long long* cnt, uint64_t stream) {
  ct_check(T, "cell_rows_dev");
  if (out_cap > 0) cr_check(R, "cell_rows_dev");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_cell_rows, dim3(launch_blocks(T.cap + 1, CR_SLOTS, "cell_rows_dev")), dim3(256), 0, st, T, R, out_cap, cnt);
  LP_HIP_CHECK(hipGetLastError());
}

void cell_reinsert_dev(const CellTab& T, const CellRows& R, int64_t n, uint64_t stream) {
  ct_check(T, "cell_reinsert_dev");
  if (n <= 0) return;
  cr_check(R, "cell_reinsert_dev");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_cell_reinsert, dim3(launch_blocks(n, 256, "cell_reinsert_dev")), dim3(256), 0, st, T, R, n);
  LP_HIP_CHECK(hipGetLastError());
}

// ---- host twins: the same table layout, one thread

static int64_t ct_claim_host(const CellTab& T, int64_t k) {
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

void cell_fold_host(const CellTab& T, const int64_t* sig, const int64_t* eff, int64_t n, int64_t line_base, int64_t W) {
  ct_check(T, "cell_fold_host");
  if (W < 1) throw std::runtime_error("cell_fold_host: the bucket width must be at least 1");
  for (int64_t i = 0; i < n; ++i) {
    const int64_t b = cell_bucket(eff[i], W);
    const int64_t s = ct_claim_host(T, cell_key(sig[i], b));
    if (s < 0) continue;
    T.sig[s] = sig[i];
    T.bucket[s] = b;
    ++T.count[s];
    T.first[s] = std::min<long long>(T.first[s], line_base + i);
  }
}

void cell_rows_host(const CellTab& T, const CellRows& R, int64_t out_cap, unsigned long long* cnt) {
  ct_check(T, "cell_rows_host");
  if (out_cap > 0) cr_check(R, "cell_rows_host");
  unsigned long long o = *cnt;
  for (int64_t s = 0; s <= T.cap; ++s) {
    if (!ct_occupied(T, s)) continue;
    if ((int64_t)o < out_cap) {
      R.sig[o] = T.sig[s];
      R.bucket[o] = T.bucket[s];
      R.count[o] = (int64_t)T.count[s];
      R.first[o] = T.first[s];
    }
    ++o;
  }
  *cnt = o;
}

void cell_reinsert_host(const CellTab& T, const CellRows& R, int64_t n) {
  ct_check(T, "cell_reinsert_host");
  if (n > 0) cr_check(R, "cell_reinsert_host");
  const unsigned long long used = T.used[0];      // (not counted here either: the caller writes it)
  for (int64_t i = 0; i < n; ++i) {
    const int64_t t = ct_claim_host(T, cell_key(R.sig[i], R.bucket[i]));
    T.used[0] = used;
    if (t < 0) continue;
    T.sig[t] = R.sig[i];
    T.bucket[t] = R.bucket[i];
    T.count[t] = (unsigned long long)R.count[i];
    T.first[t] = R.first[i];
  }
}

}  // namespace lp
