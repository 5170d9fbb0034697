// Line templates of the coverage-gap report (gaps.hip): the signature of a line is FNV-1a-64 of its
// template -- the first SIG_MAX_BYTES bytes with every [0-9A-Za-z] run that holds a digit replaced
// by one '0' and every run of space / tab by one space (log_parser_amd/golden.py line_template is
// the specification). One source for the gfx950 kernel and its host twin, as in lp_core.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lp_core.h"

namespace lp {

constexpr int SIG_MAX_BYTES = 1024;
constexpr uint64_t SIG_FNV_OFFSET = 0xcbf29ce484222325ull;
constexpr uint64_t SIG_FNV_PRIME = 0x100000001b3ull;

// a candidate of the report: an error keyword (bit0) or an exception / error class name (bit3),
// and not a stack frame (bit2) -- the bits of context_feat
LP_HD bool gap_candidate(uint8_t f) { return (f & 9) != 0 && (f & 4) == 0; }

LP_HD uint64_t sig_fold(uint64_t h, uint32_t c) { return (h ^ (uint64_t)c) * SIG_FNV_PRIME; }

// Single pass over the bytes: h is the hash of the template written so far, g the hash with the
// open token's bytes folded in as they are. A token that ends without a digit commits g; one with
// a digit folds a single '0' into h instead. Every step is a chain of selects (no branch: the lanes
// of a wave walk different lines).
//
// The walk is a chain of dependent 64-bit multiplies, so a step is arranged for depth, not for
// work: h0 = fold(h, '0') is kept up to date next to h (h does not change inside a token, so the
// fold is off the chain by the time a digit token commits), and a byte needs ONE fold on the
// chain -- of g inside a token, of the committed hash otherwise.
struct SigState {
  uint64_t h = SIG_FNV_OFFSET, g = SIG_FNV_OFFSET;
  uint64_t h0 = (SIG_FNV_OFFSET ^ (uint64_t)'0') * SIG_FNV_PRIME;   // fold(h, '0'), always
  uint32_t tok = 0;   // inside a [0-9A-Za-z] run
  uint32_t dig = 0;   // ... that has held a digit
  uint32_t sp = 0;    // the previous byte was a space or a tab
};

LP_HD void sig_step(SigState& S, uint32_t c, bool on) {
  const bool dg = c - '0' < 10u;
  const bool al = dg || ((c | 32u) - 'a' < 26u);
  const bool ws = c == ' ' || c == '\t';
  // the hash with an open token committed (no token open: h itself)
  const uint64_t hc = S.tok ? (S.dig ? S.h0 : S.g) : S.h;
  // token byte: into g (a token opens at h = hc); other byte: into the committed hash, a run of
  // spaces / tabs once as one space
  const uint64_t v = sig_fold((al && S.tok) ? S.g : hc, ws ? (uint32_t)' ' : c);
  const uint64_t hn = (ws && S.sp) ? hc : v;
  if (on) {
    S.g = al ? v : S.g;
    S.dig = al ? ((S.tok ? S.dig : 0u) | (dg ? 1u : 0u)) : 0u;
    if (!al) {                       // (a select on the device: both sides are in registers)
      S.h = hn;
      S.h0 = sig_fold(hn, '0');
    }
    S.tok = al ? 1u : 0u;
    S.sp = ws ? 1u : 0u;
  }
}

LP_HD uint64_t sig_finish(const SigState& S) { return S.tok ? (S.dig ? S.h0 : S.g) : S.h; }

#if defined(__HIP_DEVICE_COMPILE__)
// 16 bytes at the 16-byte aligned offset `off` of text[0, tbytes): one vector load when the block
// lies inside the buffer, its in-range bytes otherwise (a text without the usual padding)
__device__ __forceinline__ uint4 sig_ld16(const uint8_t* __restrict__ text, int64_t tbytes, int64_t off) {
  if (off + 16 <= tbytes) return *reinterpret_cast<const uint4*>(text + off);
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  for (int j = 0; j < 16; ++j)
    if (off + j < tbytes) w[j >> 2] |= (uint32_t)text[off + j] << (8 * (j & 3));
  return make_uint4(w[0], w[1], w[2], w[3]);
}
#endif

// signature of the line text[start, start + n) (text: 16-byte aligned on the device). Device: the
// bytes come from aligned 16-byte loads one block ahead, the lead-in of the first block masked, as
// in dfa_advance; never a byte before `text` or at / after text + tbytes.
LP_HD uint64_t line_sig_at(const uint8_t* __restrict__ text, int64_t tbytes, int64_t start, int n) {
  if (start < 0) start = 0;
  if (start > tbytes) start = tbytes;
  if (n > SIG_MAX_BYTES) n = SIG_MAX_BYTES;
  if ((int64_t)n > tbytes - start) n = (int)(tbytes - start);
  SigState S;
#if defined(__HIP_DEVICE_COMPILE__)
  if (n > 0) {
    const int sh = (int)(start & 15);
    int64_t off = start - sh;
    uint4 cur = sig_ld16(text, tbytes, off);
    for (int t0 = -sh; t0 < n; t0 += 16) {
      off += 16;
      const uint4 nxt = t0 + 16 < n ? sig_ld16(text, tbytes, off) : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int t = t0 + j;
        const uint32_t w = (j < 4) ? cur.x : (j < 8) ? cur.y : (j < 12) ? cur.z : cur.w;
        sig_step(S, (w >> (8 * (j & 3))) & 0xFFu, (t >= 0) & (t < n));
      }
      cur = nxt;
    }
  }
#else
  for (int t = 0; t < n; ++t) sig_step(S, text[start + t], true);
#endif
  return sig_finish(S);
}

LP_HD uint64_t line_sig(const uint8_t* s, int n) {
#if defined(__HIP_DEVICE_COMPILE__)
  // (a bare pointer: the aligned loads count from the pointer's own 16-byte block and end with the
  // block of the last byte -- the caller's buffer is padded as every device text is)
  const int64_t sh = (int64_t)((uintptr_t)s & 15);
  return line_sig_at(s - sh, (sh + (n > 0 ? n : 0) + 15) & ~int64_t(15), sh, n);
#else
  return line_sig_at(s, n > 0 ? n : 0, 0, n);
#endif
}

}  // namespace lp
