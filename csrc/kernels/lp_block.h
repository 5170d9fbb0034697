// Block primitives of the report kernels (gaps, gap_table, novelty, leadup, correlate, values, variants,
// timeline, trends, pauses, cadence, traces): the scans, the compaction steps and the launch geometry that
// every "one lane per line and round" kernel needs, written once. Every device piece is for blocks
// of 256 lanes (four waves of 64) and is called by ALL lanes of the block -- shuffles, ballots and
// barriers are whole-wave or whole-block -- so a caller's loop around them has a uniform trip count.
// Each .hip is its own translation unit: everything here is a template or forced inline.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <stdexcept>
#include <string>

namespace lp {

// ---- host side: the error check of a launch and the launch geometry

#define LP_HIP_CHECK(x)                                                                                         \
  do {                                                                                                          \
    hipError_t e_ = (x);                                                                                        \
    if (e_ != hipSuccess) throw std::runtime_error(std::string("HIP error: ") + hipGetErrorString(e_) + " at " #x); \
  } while (0)

// the text kernels read 16 bytes at a time
inline void check_text_aligned(const void* text, const char* who) {
  if (((uintptr_t)text & 15) != 0) throw std::runtime_error(std::string(who) + ": text must be 16-byte aligned");
}

// blocks of `per` items for n items; `what` names the items in the error
inline unsigned launch_blocks(int64_t n, int64_t per, const char* who, const char* what = "items") {
  const int64_t b = (n + per - 1) / per;
  if (b > 0x7fffffffll) throw std::runtime_error(std::string(who) + ": too many " + what + " for one launch");
  return (unsigned)b;
}

struct LineGeom {
  int per;           // lines per block: a multiple of 256, at most max_lines
  unsigned blocks;
};

// A block owns `per` consecutive lines, one lane per line and round. per_block <= 0: the default --
// enough blocks to spread a small document over the CUs (n / spread lines each, 256 at least),
// max_lines for big ones.
inline LineGeom line_geom(int64_t n, int per_block, int max_lines, const char* who, int spread = 2048) {
  int per = per_block;
  if (per <= 0) per = (int)std::min<int64_t>(max_lines, std::max<int64_t>(256, n / spread));
  per = (per + 255) / 256 * 256;
  if (per > max_lines) throw std::runtime_error(std::string(who) + ": per_block must be at most " + std::to_string(max_lines));
  return LineGeom{per, launch_blocks(n, per, who, "lines")};
}

// ---- wave (64 lanes)

// inclusive scan of a per-lane count within the wave
__device__ __forceinline__ int wave_incl_count(int c) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int v = __shfl_up(c, d, 64);
    if (lane >= d) c += v;
  }
  return c;
}

// every lane gets op over the wave's 64 values (a butterfly: op is associative and commutative)
template <class T, class Op>
__device__ __forceinline__ T wave_reduce(T x, Op op) {
#pragma unroll
  for (int d = 32; d; d >>= 1) x = op(x, __shfl_xor(x, d, 64));
  return x;
}

__device__ __forceinline__ unsigned int wave_sum(unsigned int x) {
  return wave_reduce(x, [](unsigned int a, unsigned int b) { return a + b; });
}

// Appends the lanes of `picks` (a __ballot) to the list whose length is *n -- the block's LDS list
// or an output in global memory -- with ONE atomic per wave. Returns the lane's index in the list:
// meaningful for the lanes in `picks` only.
template <class N>
__device__ __forceinline__ N wave_list_append(unsigned long long picks, N* n) {
  const int lane = threadIdx.x & 63;
  N slot = 0;
  if (picks) {                               // wave-uniform
    if (lane == 0) slot = atomicAdd(n, (N)__popcll(picks));
    slot = __shfl(slot, 0, 64);
  }
  return slot + (N)__popcll(picks & ((1ull << lane) - 1ull));
}

// ---- block (256 lanes)

// Inclusive Hillis-Steele scan of the lanes' values in s[256] over an associative `join`; returns
// the lane's EXCLUSIVE value (`identity` for lane 0) and the block's total in `total`. Its first
// barrier also orders whatever the caller wrote to LDS before the call. s is read last before the
// return: a barrier has to stand between this call and the next write of s.
template <class T, class Join>
__device__ __forceinline__ T block_scan_excl(const T& mine, const T& identity, T* s, T& total, Join join) {
  const int t = threadIdx.x;
  s[t] = mine;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    T x = s[t];
    if (t >= d) x = join(s[t - d], x);
    __syncthreads();
    s[t] = x;
    __syncthreads();
  }
  total = s[255];
  return t ? s[t - 1] : identity;
}

// Exclusive scan of a per-lane count over the block: shuffles within the wave, the four wave totals
// through s_wave[4]. Returns the lane's offset and the block's total in `total`. ONE barrier,
// between the write of s_wave and its reads; it also orders whatever the caller wrote to LDS
// before the call. A barrier has to stand between this call and the next write of s_wave.
__device__ __forceinline__ int block_excl_count(int c, int* s_wave, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int incl = wave_incl_count(c);
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  int off = incl - c;
  total = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int t = s_wave[w];
    off += w < wave ? t : 0;
    total += t;
  }
  return off;
}

// Lane 0 reserves `total` output rows (block-uniform, or at least lane 0's value) with ONE global
// atomic on *cnt and publishes the base through *s_base; every lane returns it. The barrier stands
// after lane 0's write of *s_base and before every lane's read of it. It also orders the LDS writes
// of all lanes before the call -- the staged rows, the block's counters -- before the reads after
// it: the copy-out needs no barrier of its own. A barrier has to stand between the read here and
// the next write of *s_base (in a loop of rounds: the one in block_excl_count).
__device__ __forceinline__ int64_t block_reserve(unsigned long long* cnt, int total, long long* s_base) {
  if (threadIdx.x == 0) *s_base = total ? (long long)atomicAdd(cnt, (unsigned long long)total) : 0;
  __syncthreads();
  return *s_base;
}

}  // namespace lp
