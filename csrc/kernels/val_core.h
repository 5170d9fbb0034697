// Numeric fields of a line for the values report (values.hip). The *fields* of a line are the
// digit-holding [0-9A-Za-z] runs of its first SIG_MAX_BYTES bytes -- exactly the tokens that the
// template of gaps_core.h turns into '0' -- that start at or behind the line's stamp end
// (ts_core.h line_ts_span_at), numbered j = 0, 1, ... in byte order; the first VAL_PER_LINE count. A
// field *has a value* where its token is [0-9]{1,9}[A-Za-z]{0,3} from start to end: the integer of
// the digit prefix (log_parser_amd/golden.py line_values is the specification). One source for the
// gfx950 kernel and its host twin, as key_core.h is.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gaps_core.h"
#include "lp_core.h"
#include "ts_core.h"

namespace lp {

constexpr int VAL_PER_LINE = 8;
constexpr uint32_t VAL_MAX_DIGITS = 9;     // 0 .. 999,999,999: below 2^30
constexpr uint32_t VAL_MAX_LETTERS = 3;    // ms, MB, rd, KiB

// the group key of field j of a template: a 64-bit mix of (signature, j)
LP_HD uint64_t val_key(uint64_t sig, int j) { return (sig ^ (uint64_t)(j + 1)) * SIG_FNV_PRIME; }

// The values of one line: slot j is the value of field j where bit j of `mask` is set. Eight slots
// that are only ever indexed by the constant of an unrolled loop: on the device they are
// registers, never scratch.
struct ValList {
  int32_t v[VAL_PER_LINE] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t mask = 0;
};

// slot j = val (j < VAL_PER_LINE): selects over the eight slots, as in key_insert
LP_HD void val_set(ValList& L, uint32_t j, int32_t val) {
#pragma unroll
  for (int k = 0; k < VAL_PER_LINE; ++k) L.v[k] = ((uint32_t)k == j) ? val : L.v[k];
  L.mask |= 1u << j;
}

// The open token next to SigState's `tok` (a token is open) and `dig` (it has held a digit): does it
// start before the stamp end, how many digits lead it, how many letters follow them, has its shape
// failed, and the value of the digits so far. `field`: digit-holding tokens at or behind the stamp
// end that have ended -- the number of the next one.
struct ValState {
  uint32_t hid = 0;
  uint32_t nd = 0;
  uint32_t nl = 0;
  uint32_t bad = 0;
  uint32_t val = 0;
  uint32_t field = 0;
};

// the token that SigState S describes has ended: a field if it held a digit and is not hidden
LP_HD void val_close(const ValState& V, ValList& L, uint32_t field) {
  if (field < (uint32_t)VAL_PER_LINE && !V.bad) val_set(L, field, (int32_t)V.val);
}

// One byte, BEFORE sig_step of the same byte: `tok` / `dig` are S.tok / S.dig of the bytes so far.
// t: the byte's offset in the line, q: the stamp end.
LP_HD void val_step(ValState& V, ValList& L, uint32_t tok, uint32_t dig, uint32_t c, int t, int q, bool on) {
  const bool dg = c - '0' < 10u;
  const bool al = dg || ((c | 32u) - 'a' < 26u);
  // a token ends on the first other byte: a field if it held a digit and is not hidden. What the
  // branch does inside is selects
  const bool ends = on && !al && tok != 0u && dig != 0u && V.hid == 0u;
  if (ends) val_close(V, L, V.field);
  V.field += ends ? 1u : 0u;
  if (on && al) {                       // (selects on the device: everything is in registers)
    // a token byte: the token opens here (digits 0, letters 0) or goes on: digits, then at most
    // three letters. A digit behind a letter (every digit-holding token that starts with a letter
    // has one), a tenth digit or a fourth letter: no value. (val wraps from the tenth digit on: bad
    // by then)
    const bool in = tok != 0u;
    const uint32_t nd = in ? V.nd : 0u, nl = in ? V.nl : 0u, val = in ? V.val : 0u, bad = in ? V.bad : 0u;
    const bool late = dg && nl != 0u;
    V.hid = in ? V.hid : (t < q ? 1u : 0u);
    V.nd = nd + (dg ? 1u : 0u);
    V.nl = nl + (dg ? 0u : 1u);
    V.val = dg ? val * 10u + (c - '0') : val;
    V.bad = bad | ((late || V.nd > VAL_MAX_DIGITS || V.nl > VAL_MAX_LETTERS) ? 1u : 0u);
  }
}

// Signature and values of the line text[start, start + n) (text: 16-byte aligned on the device):
// ONE forward pass, sig_step and the value state machine side by side. Device: the bytes come from
// aligned 16-byte loads one block ahead exactly as in line_sig_at; never a byte before `text` or at
// / after text + tbytes. The stamp end comes first (line_ts_span_at re-reads at most TS_MAX_BYTES
// bytes that the walk is about to read anyway). A token still open at the end of the walk -- the
// end of the line, or byte SIG_MAX_BYTES -- ends there.
LP_HD uint64_t line_vals_at(const uint8_t* __restrict__ text, int64_t tbytes, int64_t start, int n, ValList& L) {
  if (start < 0) start = 0;
  if (start > tbytes) start = tbytes;
  const int q = line_ts_span_at(text, tbytes, start, n);
  if (n > SIG_MAX_BYTES) n = SIG_MAX_BYTES;
  if ((int64_t)n > tbytes - start) n = (int)(tbytes - start);
  SigState S;
  ValState V;
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
        const uint32_t c = (w >> (8 * (j & 3))) & 0xFFu;
        const bool on = (t >= 0) & (t < n);
        val_step(V, L, S.tok, S.dig, c, t, q, on);
        sig_step(S, c, on);
      }
      cur = nxt;
    }
  }
#else
  for (int t = 0; t < n; ++t) {
    val_step(V, L, S.tok, S.dig, text[start + t], t, q, true);
    sig_step(S, text[start + t], true);
  }
#endif
  if (S.tok && S.dig && !V.hid) val_close(V, L, V.field);
  return sig_finish(S);
}

}  // namespace lp
