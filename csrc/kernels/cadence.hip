// Cadence report: which line templates come at a steady beat, and where did one miss beats? The
// input is what k_line_stamps gives per line (stamp, template signature). The stamped lines of ONE
// signature in line order are j_0 < j_1 < ...; the beat k is ts[j_k] - ts[j_{k-1}] with the
// from-line j_{k-1} and the to-line j_k. A beat below 0 is a backward beat and only counted. That
// is a group-by-key with order inside the group; everything is exact int64 and the same on every run.
//
// A *row* summarises consecutive stamped occurrences of one signature (CD_COLS columns): its beats,
// and the first and last (line, stamp). Two rows of one signature, a before b, join associatively:
// the border beat b.first - a.last enters the counts (cd_join). One stamped line is a row without a
// beat, so every kernel and the host twins use the one join.
//
//   k_cd_tile    one block per 2,048 consecutive lines: a bitonic sort of (stamped first, signature,
//                line) in LDS puts consecutive occurrences side by side; each computes its beat and
//                writes beat / bucket at its own line; a segmented scan (flagged join) gives one row
//                per distinct signature of the tile, appended with one global atomic per block
//   (torch)      state rows and tile rows sorted by first line, then stably by signature: the order
//                the atomic gave is gone
//   k_cdl_tiles  per block of 256 sorted rows: the flagged aggregate, the number of segment ends
//   k_cdl_prefix one block: the aggregates become exclusive prefixes, the counts row offsets
//   k_cdl_emit   one output row per signature at its offset (sorted by signature: the new state);
//                a row that follows one of its signature is the first of its tile or run, so its
//                first line gets the border beat the tile kernel had to leave open
//
// log_parser_amd/cadence.py drives them; log_parser_amd/golden.py cadence is the specification.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "lp_api.h"
#include "lp_block.h"
#include "lp_core.h"
#include "ts_core.h"

namespace lp {

namespace {
using ull = unsigned long long;
}

constexpr int CD_PER_LANE = 8;                       // consecutive sorted places of one lane
constexpr int CD_TILE = 256 * CD_PER_LANE;           // lines of one block of k_cd_tile
constexpr int CDL_ROWS = 256;                        // rows of one block of the link kernels
constexpr int CDL_WORDS = 14;                        // words of a block's entry in the link workspace

// consecutive stamped occurrences of one signature; first_line < 0: none (the join's identity).
// lines = beats + back + 1: every neighbouring pair is one beat
struct CdRow {
  int64_t beats, back;                 // forward beats, backward beats
  int64_t sum, mn, mx;                 // of the forward beats (mn INT64_MAX, mx -1: none)
  int64_t mx_from, mx_to, mx_to_ts;    // the lines of the first largest beat, the stamp of its to-line
  int64_t first_line, first_ts, last_line, last_ts;
};

struct CdSeg {
  int64_t flag;              // a segment starts inside: `row` covers the last segment only
  CdRow row;
};

LP_HD CdRow cd_none() { return CdRow{0, 0, 0, INT64_MAX, -1, -1, -1, 0, -1, 0, -1, 0}; }

LP_HD CdRow cd_single(int64_t line, int64_t ts) { return CdRow{0, 0, 0, INT64_MAX, -1, -1, -1, 0, line, ts, line, ts}; }

// to - from without signed overflow (the caller keeps stamps within +-2^61: no beat wraps)
LP_HD int64_t cd_step(int64_t from, int64_t to) { return (int64_t)((uint64_t)to - (uint64_t)from); }

// bucket of a beat >= 0: its bit length (pauses' intervals); TS_NONE for a backward beat or none
LP_HD int64_t cd_bucket(int64_t beat) {
  if (beat == TS_NONE || beat < 0) return TS_NONE;
  return beat == 0 ? 0 : 64 - __builtin_clzll((ull)beat);
}

// a, then b, of ONE signature. Among equal largest beats the earliest stays: a's, the border, b's
LP_HD CdRow cd_join(const CdRow& a, const CdRow& b) {
  if (a.first_line < 0) return b;
  if (b.first_line < 0) return a;
  CdRow r = a;
  r.beats += b.beats;
  r.back += b.back;
  r.sum = (int64_t)((uint64_t)a.sum + (uint64_t)b.sum);
  r.mn = b.mn < a.mn ? b.mn : a.mn;
  const int64_t beat = cd_step(a.last_ts, b.first_ts);
  if (beat < 0) {
    ++r.back;
  } else {
    ++r.beats;
    r.sum = (int64_t)((uint64_t)r.sum + (uint64_t)beat);
    r.mn = beat < r.mn ? beat : r.mn;
    if (beat > r.mx) {
      r.mx = beat;
      r.mx_from = a.last_line;
      r.mx_to = b.first_line;
      r.mx_to_ts = b.first_ts;
    }
  }
  if (b.mx > r.mx) {
    r.mx = b.mx;
    r.mx_from = b.mx_from;
    r.mx_to = b.mx_to;
    r.mx_to_ts = b.mx_to_ts;
  }
  r.last_line = b.last_line;
  r.last_ts = b.last_ts;
  return r;
}

// the flagged operator of the segmented scans: b after a
LP_HD CdSeg cd_seg_join(const CdSeg& a, const CdSeg& b) {
  if (b.flag) return b;
  return CdSeg{a.flag, cd_join(a.row, b.row)};
}

LP_HD void cd_put(int64_t* rows, int64_t cap, int64_t o, int64_t sig, const CdRow& r) {
  rows[CD_SIG * cap + o] = sig;
  rows[CD_LINES * cap + o] = r.beats + r.back + 1;
  rows[CD_BEATS * cap + o] = r.beats;
  rows[CD_BACKWARD * cap + o] = r.back;
  rows[CD_SUM * cap + o] = r.sum;
  rows[CD_MIN * cap + o] = r.mn;
  rows[CD_MAX * cap + o] = r.mx;
  rows[CD_MAX_FROM * cap + o] = r.mx_from;
  rows[CD_MAX_TO * cap + o] = r.mx_to;
  rows[CD_FIRST_LINE * cap + o] = r.first_line;
  rows[CD_LAST_LINE * cap + o] = r.last_line;
  rows[CD_LAST_TS * cap + o] = r.last_ts;
  rows[CD_FIRST_TS * cap + o] = r.first_ts;
  rows[CD_MAX_TO_TS * cap + o] = r.mx_to_ts;
}

LP_HD CdRow cd_get(const int64_t* rows, int64_t n, int64_t i) {
  return CdRow{rows[CD_BEATS * n + i],      rows[CD_BACKWARD * n + i],   rows[CD_SUM * n + i],       rows[CD_MIN * n + i],
               rows[CD_MAX * n + i],        rows[CD_MAX_FROM * n + i],   rows[CD_MAX_TO * n + i],    rows[CD_MAX_TO_TS * n + i],
               rows[CD_FIRST_LINE * n + i], rows[CD_FIRST_TS * n + i],   rows[CD_LAST_LINE * n + i], rows[CD_LAST_TS * n + i]};
}

// (stamped first, signature as a signed number, line): a total order, no two keys are equal
__device__ __forceinline__ bool cd_less(long long sa, unsigned short ia, long long sb, unsigned short ib) {
  const int fa = ia >> 15, fb = ib >> 15;
  if (fa != fb) return fa < fb;
  if (sa != sb) return sa < sb;
  return ia < ib;
}

__global__ __launch_bounds__(256) void k_cd_tile(CadenceTileArgs A) {
  __shared__ long long s_sig[CD_TILE];            // by sorted place
  __shared__ unsigned short s_idx[CD_TILE];       // by sorted place: the line of the tile, bit 15: unstamped
  __shared__ long long s_ts[CD_TILE];             // by line of the tile
  __shared__ CdSeg s_scan[256];
  __shared__ int s_wave[4];
  __shared__ long long s_base;
  const int t = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * CD_TILE;
  for (int j = t; j < CD_TILE; j += 256) {
    const int64_t i = base + j;
    const int64_t ts = i < A.L ? A.ts[i] : TS_NONE;
    s_ts[j] = ts;
    s_sig[j] = ts != TS_NONE ? A.sig[i] : 0;
    s_idx[j] = (unsigned short)(j | (ts == TS_NONE ? 0x8000 : 0));
    if (i < A.L && ts == TS_NONE) {
      A.beat[i] = TS_NONE;
      A.bkt[i] = TS_NONE;
    }
  }
  __syncthreads();
  // bitonic sort of the 2,048 keys, four compare-exchanges per lane and step
  for (int k = 2; k <= CD_TILE; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int q = t; q < CD_TILE / 2; q += 256) {
        const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1));
        const int p = i | j;
        const long long si = s_sig[i], sp = s_sig[p];
        const unsigned short ii = s_idx[i], ip = s_idx[p];
        const bool up = (i & k) == 0;
        if (up ? cd_less(sp, ip, si, ii) : cd_less(si, ii, sp, ip)) {
          s_sig[i] = sp;
          s_sig[p] = si;
          s_idx[i] = ip;
          s_idx[p] = ii;
        }
      }
      __syncthreads();
    }
  }
  // the lane's places [p0, p0 + 8): the beats of the ones that follow their kind, the lane's aggregate
  const int p0 = t * CD_PER_LANE;
  const int64_t g0 = A.line_base + base;
  CdSeg agg{0, cd_none()};
  int ends = 0;
#pragma unroll
  for (int j = 0; j < CD_PER_LANE; ++j) {
    const int p = p0 + j;
    const unsigned short ix = s_idx[p];
    if (ix >> 15) break;                        // the unstamped lines sort last
    const long long sg = s_sig[p];
    const int64_t ts = s_ts[ix];
    const bool head = p == 0 || s_sig[p - 1] != sg;
    const CdRow one = cd_single(g0 + ix, ts);
    int64_t beat = TS_NONE;
    if (head) {
      agg = CdSeg{1, one};
    } else {
      agg.row = cd_join(agg.row, one);
      beat = cd_step(s_ts[s_idx[p - 1]], ts);
    }
    A.beat[base + ix] = beat;
    A.bkt[base + ix] = cd_bucket(beat);
    ends += (p + 1 == CD_TILE || (s_idx[p + 1] >> 15) || s_sig[p + 1] != sg) ? 1 : 0;
  }
  CdSeg total;
  const CdSeg excl = block_scan_excl(agg, CdSeg{0, cd_none()}, s_scan, total,
                                     [](const CdSeg& a, const CdSeg& b) { return cd_seg_join(a, b); });
  int rows;
  const int off = block_excl_count(ends, s_wave, rows);
  int64_t o = block_reserve(A.cnt, rows, &s_base) + off;
  if (!ends) return;
  CdRow cur = excl.row;
#pragma unroll
  for (int j = 0; j < CD_PER_LANE; ++j) {
    const int p = p0 + j;
    const unsigned short ix = s_idx[p];
    if (ix >> 15) break;
    const long long sg = s_sig[p];
    const bool head = p == 0 || s_sig[p - 1] != sg;
    const CdRow one = cd_single(g0 + ix, s_ts[ix]);
    cur = head ? one : cd_join(cur, one);
    if (p + 1 == CD_TILE || (s_idx[p + 1] >> 15) || s_sig[p + 1] != sg) {
      if (o < A.cap) cd_put(A.rows, A.cap, o, sg, cur);     // over capacity: counted, the caller reruns
      ++o;
    }
  }
}

// ---- the link: a segmented reduce over rows sorted by (signature, first line)

// row r of the sorted rows as the scan's element: does it start a segment, does it end one
__device__ __forceinline__ CdSeg cdl_load(const int64_t* __restrict__ in, int64_t R, int64_t r, bool& end) {
  end = false;
  if (r >= R) return CdSeg{0, cd_none()};
  const int64_t sg = in[CD_SIG * R + r];
  end = r + 1 == R || in[CD_SIG * R + r + 1] != sg;
  return CdSeg{(r == 0 || in[CD_SIG * R + r - 1] != sg) ? 1 : 0, cd_get(in, R, r)};
}

__device__ __forceinline__ void cdl_store(int64_t* w, const CdSeg& s) {
  w[0] = s.flag;
  w[1] = s.row.beats; w[2] = s.row.back; w[3] = s.row.sum; w[4] = s.row.mn; w[5] = s.row.mx;
  w[6] = s.row.mx_from; w[7] = s.row.mx_to; w[8] = s.row.mx_to_ts;
  w[9] = s.row.first_line; w[10] = s.row.first_ts; w[11] = s.row.last_line; w[12] = s.row.last_ts;
}

__device__ __forceinline__ CdSeg cdl_fetch(const int64_t* w) {
  return CdSeg{w[0], CdRow{w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8], w[9], w[10], w[11], w[12]}};
}

// tmp: CDL_WORDS words per block: [0..12] its aggregate, then its incoming prefix; [13] its segment
// ends, then the offset of its first output row
__global__ __launch_bounds__(256) void k_cdl_tiles(const int64_t* __restrict__ in, int64_t R, int64_t* __restrict__ tmp) {
  __shared__ CdSeg s_scan[256];
  __shared__ int s_wave[4];
  bool end;
  const CdSeg mine = cdl_load(in, R, (int64_t)blockIdx.x * CDL_ROWS + threadIdx.x, end);
  CdSeg total;
  block_scan_excl(mine, CdSeg{0, cd_none()}, s_scan, total, [](const CdSeg& a, const CdSeg& b) { return cd_seg_join(a, b); });
  int ends;
  block_excl_count(end ? 1 : 0, s_wave, ends);
  if (threadIdx.x == 0) {
    cdl_store(tmp + (int64_t)blockIdx.x * CDL_WORDS, total);
    tmp[(int64_t)blockIdx.x * CDL_WORDS + 13] = ends;
  }
}

// one block: lane t owns the blocks [t * per, (t + 1) * per). head[0]: the output rows
__global__ __launch_bounds__(256) void k_cdl_prefix(int64_t* __restrict__ tmp, int64_t nb, int64_t* __restrict__ head) {
  __shared__ CdSeg s_scan[256];
  __shared__ long long s_sum[256];
  const int t = threadIdx.x;
  const int64_t per = (nb + 255) / 256;
  const int64_t a = (int64_t)t * per, b = a + per < nb ? a + per : nb;
  CdSeg p{0, cd_none()};
  long long c = 0;
  for (int64_t k = a; k < b; ++k) {
    p = cd_seg_join(p, cdl_fetch(tmp + k * CDL_WORDS));
    c += tmp[k * CDL_WORDS + 13];
  }
  CdSeg total;
  p = block_scan_excl(p, CdSeg{0, cd_none()}, s_scan, total, [](const CdSeg& x, const CdSeg& y) { return cd_seg_join(x, y); });
  long long sum;
  long long off = block_scan_excl(c, 0ll, s_sum, sum, [](long long x, long long y) { return x + y; });
  for (int64_t k = a; k < b; ++k) {
    const CdSeg own = cdl_fetch(tmp + k * CDL_WORDS);
    const long long n = tmp[k * CDL_WORDS + 13];
    cdl_store(tmp + k * CDL_WORDS, p);
    tmp[k * CDL_WORDS + 13] = off;
    p = cd_seg_join(p, own);
    off += n;
  }
  if (t == 255) head[0] = sum;
}

__global__ __launch_bounds__(256) void k_cdl_emit(CadenceLinkArgs A) {
  __shared__ CdSeg s_scan[256];
  __shared__ int s_wave[4];
  const int64_t r = (int64_t)blockIdx.x * CDL_ROWS + threadIdx.x;
  bool end;
  const CdSeg mine = cdl_load(A.in, A.R, r, end);
  CdSeg total;
  CdSeg excl = block_scan_excl(mine, CdSeg{0, cd_none()}, s_scan, total,
                               [](const CdSeg& a, const CdSeg& b) { return cd_seg_join(a, b); });
  excl = cd_seg_join(cdl_fetch(A.tmp + (int64_t)blockIdx.x * CDL_WORDS), excl);
  int ends;
  const int off = block_excl_count(end ? 1 : 0, s_wave, ends);
  if (r >= A.R) return;
  if (!mine.flag) {
    // the row follows one of its signature: the border beat belongs to its first line, if that is of this run
    const int64_t i = mine.row.first_line - A.line_base;
    if (i >= 0 && i < A.L) {
      const int64_t beat = cd_step(A.in[CD_LAST_TS * A.R + r - 1], mine.row.first_ts);
      A.beat[i] = beat;
      A.bkt[i] = cd_bucket(beat);
    }
  }
  if (end) {
    const int64_t o = A.tmp[(int64_t)blockIdx.x * CDL_WORDS + 13] + off;
    if (o < A.cap) cd_put(A.out, A.cap, o, A.in[CD_SIG * A.R + r], cd_seg_join(excl, mine).row);
  }
}

static int64_t cd_tiles_of(int64_t L) { return (std::max<int64_t>(L, 0) + CD_TILE - 1) / CD_TILE; }
static int64_t cdl_blocks_of(int64_t R) { return (std::max<int64_t>(R, 0) + CDL_ROWS - 1) / CDL_ROWS; }

int64_t cadence_link_tmp_words(int64_t R) { return CDL_WORDS * cdl_blocks_of(R); }

static void cd_tile_check(const CadenceTileArgs& A, const char* who) {
  if (A.L < 0 || cd_tiles_of(A.L) > 0x7fffffffll) throw std::runtime_error(std::string(who) + ": too many lines for one launch");
  if (A.line_base < 0 || A.line_base > INT64_MAX - A.L) throw std::runtime_error(std::string(who) + ": line_base out of range");
  if (A.L && (!A.ts || !A.sig || !A.beat || !A.bkt)) throw std::runtime_error(std::string(who) + ": missing column");
  if (A.cap < 0 || (A.cap && !A.rows) || !A.cnt) throw std::runtime_error(std::string(who) + ": missing output");
}

static void cd_link_check(const CadenceLinkArgs& A, const char* who) {
  if (A.R < 0 || cdl_blocks_of(A.R) > 0x7fffffffll) throw std::runtime_error(std::string(who) + ": too many rows for one launch");
  if (A.L < 0 || A.line_base < 0 || A.line_base > INT64_MAX - A.L) throw std::runtime_error(std::string(who) + ": line_base out of range");
  if (A.L && (!A.beat || !A.bkt)) throw std::runtime_error(std::string(who) + ": missing column");
  if (!A.head || A.cap < 0 || (A.R && !A.in) || (A.cap && !A.out)) throw std::runtime_error(std::string(who) + ": missing rows");
}

void cadence_tile_dev(const CadenceTileArgs& A, uint64_t stream) {
  cd_tile_check(A, "cadence_tile_dev");
  if (A.L <= 0) return;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_cd_tile, dim3((unsigned)cd_tiles_of(A.L)), dim3(256), 0, st, A);
  LP_HIP_CHECK(hipGetLastError());
}

void cadence_link_dev(const CadenceLinkArgs& A, uint64_t stream) {
  cd_link_check(A, "cadence_link_dev");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (A.R <= 0) {
    LP_HIP_CHECK(hipMemsetAsync(A.head, 0, sizeof(int64_t), st));
    return;
  }
  if (!A.tmp) throw std::runtime_error("cadence_link_dev: missing workspace");
  const int64_t nb = cdl_blocks_of(A.R);
  hipLaunchKernelGGL(k_cdl_tiles, dim3((unsigned)nb), dim3(256), 0, st, A.in, A.R, A.tmp);
  LP_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_cdl_prefix, dim3(1), dim3(256), 0, st, A.tmp, nb, A.head);
  LP_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_cdl_emit, dim3((unsigned)nb), dim3(256), 0, st, A);
  LP_HIP_CHECK(hipGetLastError());
}

// ---- host twins: one walk in line order with a dict per tile; one walk over the sorted rows

void cadence_tile_host(const CadenceTileArgs& A) {
  cd_tile_check(A, "cadence_tile_host");
  int64_t o = (int64_t)*A.cnt;
  std::unordered_map<int64_t, size_t> at;
  std::vector<std::pair<int64_t, CdRow>> rows;
  for (int64_t base = 0; base < A.L; base += CD_TILE) {
    const int64_t end = std::min<int64_t>(A.L, base + CD_TILE);
    at.clear();
    rows.clear();
    for (int64_t i = base; i < end; ++i) {
      A.beat[i] = A.bkt[i] = TS_NONE;
      if (A.ts[i] == TS_NONE) continue;
      const CdRow one = cd_single(A.line_base + i, A.ts[i]);
      auto it = at.find(A.sig[i]);
      if (it == at.end()) {
        at.emplace(A.sig[i], rows.size());
        rows.emplace_back(A.sig[i], one);
        continue;
      }
      CdRow& r = rows[it->second].second;
      A.beat[i] = cd_step(r.last_ts, A.ts[i]);
      A.bkt[i] = cd_bucket(A.beat[i]);
      r = cd_join(r, one);
    }
    for (const auto& sr : rows) {                 // in the order of their first lines
      if (o < A.cap) cd_put(A.rows, A.cap, o, sr.first, sr.second);
      ++o;
    }
  }
  *A.cnt = (unsigned long long)o;
}

void cadence_link_host(const CadenceLinkArgs& A) {
  cd_link_check(A, "cadence_link_host");
  int64_t o = 0;
  CdRow cur = cd_none();
  for (int64_t r = 0; r < A.R; ++r) {
    const int64_t sg = A.in[CD_SIG * A.R + r];
    const CdRow mine = cd_get(A.in, A.R, r);
    if (r == 0 || A.in[CD_SIG * A.R + r - 1] != sg) {
      cur = mine;
    } else {
      const int64_t i = mine.first_line - A.line_base;
      if (i >= 0 && i < A.L) {
        A.beat[i] = cd_step(cur.last_ts, mine.first_ts);
        A.bkt[i] = cd_bucket(A.beat[i]);
      }
      cur = cd_join(cur, mine);
    }
    if (r + 1 == A.R || A.in[CD_SIG * A.R + r + 1] != sg) {
      if (o < A.cap) cd_put(A.out, A.cap, o, sg, cur);
      ++o;
    }
  }
  A.head[0] = o;
}

}  // namespace lp
