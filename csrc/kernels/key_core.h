// Keys of a line for the correlation report (correlate.hip): a key token is a maximal [0-9A-Za-z]
// run of the line's first SIG_MAX_BYTES bytes whose length is min_len .. KEY_MAX_LEN and that holds
// a digit -- a request id, a trace id, a pod hash, an address. Its key is FNV-1a-64 (the constants
// of gaps_core.h) over the token's bytes with ASCII letters lowered; the keys of a line are its
// first KEY_PER_LINE distinct keys in byte order (log_parser_amd/golden.py line_keys is the
// specification). One source for the gfx950 kernel and its host twin, as gaps_core.h is.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gaps_core.h"
#include "lp_core.h"

namespace lp {

constexpr int KEY_MIN_LEN_LO = 4;    // the smallest min_len a caller may ask for (the largest: KEY_MAX_LEN)
constexpr int KEY_MAX_LEN = 64;      // a longer run is a blob, not an id
constexpr int KEY_PER_LINE = 8;

// The key list of one line. Eight slots that are only ever indexed by the constant of an unrolled
// loop: on the device they are registers, never scratch.
struct KeyList {
  int64_t k[KEY_PER_LINE] = {0, 0, 0, 0, 0, 0, 0, 0};
  int n = 0;
};

// insert `key` unless the list holds it or is full: selects over the eight slots
LP_HD void key_insert(KeyList& K, int64_t key) {
  bool dup = false;
#pragma unroll
  for (int j = 0; j < KEY_PER_LINE; ++j) dup = dup || (j < K.n && K.k[j] == key);
  const bool ins = !dup && K.n < KEY_PER_LINE;
#pragma unroll
  for (int j = 0; j < KEY_PER_LINE; ++j) K.k[j] = (ins && j == K.n) ? key : K.k[j];
  K.n += ins ? 1 : 0;
}

// The open token: its hash so far, its length (counted up to KEY_MAX_LEN + 1: longer is longer) and
// whether it has held a digit. One dependent 64-bit multiply per byte, as in sig_step.
struct KeyState {
  uint64_t h = SIG_FNV_OFFSET;
  uint32_t len = 0;   // 0: no token open
  uint32_t dig = 0;
};

LP_HD bool key_qualifies(const KeyState& S, int min_len) {
  return S.dig != 0 && S.len >= (uint32_t)min_len && S.len <= (uint32_t)KEY_MAX_LEN;
}

LP_HD void key_step(KeyState& S, KeyList& K, uint32_t c, bool on, int min_len) {
  const bool dg = c - '0' < 10u;
  const bool al = dg || ((c | 32u) - 'a' < 26u);
  // a token ends on the first other byte. Few tokens qualify, so the insert is a branch that a
  // wave mostly skips; what it does inside is selects
  if (on && !al && key_qualifies(S, min_len)) key_insert(K, (int64_t)S.h);
  if (on) {
    // (c | 32 lowers a letter and leaves a digit as it is: both ranges have or get bit 5)
    const uint64_t v = sig_fold(S.len ? S.h : SIG_FNV_OFFSET, c | 32u);
    S.h = al ? v : S.h;
    S.dig = al ? ((S.len ? S.dig : 0u) | (dg ? 1u : 0u)) : 0u;
    const uint32_t grown = S.len < (uint32_t)KEY_MAX_LEN + 1u ? S.len + 1u : S.len;
    S.len = al ? grown : 0u;
  }
}

// The keys of the line text[start, start + n) (text: 16-byte aligned on the device). Device: the
// bytes come from aligned 16-byte loads one block ahead exactly as in line_sig_at; never a byte
// before `text` or at / after text + tbytes. A run still open at the end of the walk -- the end of
// the line, or byte SIG_MAX_BYTES -- ends there.
LP_HD void line_keys_at(const uint8_t* __restrict__ text, int64_t tbytes, int64_t start, int n, int min_len,
                        KeyList& K) {
  if (start < 0) start = 0;
  if (start > tbytes) start = tbytes;
  if (n > SIG_MAX_BYTES) n = SIG_MAX_BYTES;
  if ((int64_t)n > tbytes - start) n = (int)(tbytes - start);
  KeyState S;
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
        key_step(S, K, (w >> (8 * (j & 3))) & 0xFFu, (t >= 0) & (t < n), min_len);
      }
      cur = nxt;
    }
  }
#else
  for (int t = 0; t < n; ++t) key_step(S, K, text[start + t], true, min_len);
#endif
  if (key_qualifies(S, min_len)) key_insert(K, (int64_t)S.h);
}

// ---- with the place of every token (spans.hip): the list beside KeyList. Slot j holds the token of
// K.k[j] as (offset in the line) | (length << KEY_POS_LEN_SHIFT): the offset is below SIG_MAX_BYTES, the
// length at most KEY_MAX_LEN. Indexed by unrolled constants only, as KeyList is.
constexpr int KEY_POS_LEN_SHIFT = 10;
constexpr int32_t KEY_POS_OFF_MASK = (1 << KEY_POS_LEN_SHIFT) - 1;

struct KeyPosList {
  int32_t p[KEY_PER_LINE] = {0, 0, 0, 0, 0, 0, 0, 0};
};

LP_HD int32_t key_pos_pack(int off, uint32_t len) { return (int32_t)off | (int32_t)(len << KEY_POS_LEN_SHIFT); }

// key_insert that also notes where the token stands
LP_HD void key_insert_at(KeyList& K, KeyPosList& P, int64_t key, int32_t pos) {
  bool dup = false;
#pragma unroll
  for (int j = 0; j < KEY_PER_LINE; ++j) dup = dup || (j < K.n && K.k[j] == key);
  const bool ins = !dup && K.n < KEY_PER_LINE;
#pragma unroll
  for (int j = 0; j < KEY_PER_LINE; ++j) {
    const bool here = ins && j == K.n;
    K.k[j] = here ? key : K.k[j];
    P.p[j] = here ? pos : P.p[j];
  }
  K.n += ins ? 1 : 0;
}

// key_step for the byte at offset t of the line: a token that ends here stands at [t - len, t)
LP_HD void key_step_at(KeyState& S, KeyList& K, KeyPosList& P, uint32_t c, int t, bool on, int min_len) {
  const bool dg = c - '0' < 10u;
  const bool al = dg || ((c | 32u) - 'a' < 26u);
  if (on && !al && key_qualifies(S, min_len)) key_insert_at(K, P, (int64_t)S.h, key_pos_pack(t - (int)S.len, S.len));
  if (on) {
    const uint64_t v = sig_fold(S.len ? S.h : SIG_FNV_OFFSET, c | 32u);
    S.h = al ? v : S.h;
    S.dig = al ? ((S.len ? S.dig : 0u) | (dg ? 1u : 0u)) : 0u;
    const uint32_t grown = S.len < (uint32_t)KEY_MAX_LEN + 1u ? S.len + 1u : S.len;
    S.len = al ? grown : 0u;
  }
}

}  // namespace lp
