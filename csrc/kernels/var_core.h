// Variable tokens of a line for the variants report (variants.hip). The *fields* of a line are
// val_core.h's: the digit-holding [0-9A-Za-z] runs of its first SIG_MAX_BYTES bytes that start at
// or behind the line's stamp end, numbered j = 0, 1, ... in byte order; the first VAL_PER_LINE
// count. Here a field counts whether or not it reads as a number, and its *value* is the
// FNV-1a-64 hash (the constants of gaps_core.h) of the token's bytes as they are -- case is kept
// (log_parser_amd/golden.py line_fields / var_hash is the specification). One source for the
// gfx950 kernel and its host twin, as val_core.h is.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gaps_core.h"
#include "lp_core.h"
#include "ts_core.h"
#include "val_core.h"

namespace lp {

// The value hashes of one line: slot j is the hash of field j where bit j of `mask` is set. Eight
// slots that are only ever indexed by the constant of an unrolled loop, as ValList's: registers
// on the device, never scratch.
struct VarList {
  uint64_t v[VAL_PER_LINE] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t mask = 0;
};

// slot j = h (j < VAL_PER_LINE): selects over the eight slots, as val_set
LP_HD void var_set(VarList& L, uint32_t j, uint64_t h) {
#pragma unroll
  for (int k = 0; k < VAL_PER_LINE; ++k) L.v[k] = ((uint32_t)k == j) ? h : L.v[k];
  L.mask |= 1u << j;
}

// The open token next to SigState's `tok` / `dig`: does it start before the stamp end, and the
// hash of its bytes so far. `field`: digit-holding tokens at or behind the stamp end that have
// ended -- the number of the next one (it counts on past VAL_PER_LINE; those fill no slot).
struct VarState {
  uint32_t hid = 0;
  uint32_t field = 0;
  uint64_t th = SIG_FNV_OFFSET;
};

// the token that SigState describes has ended and is a field
LP_HD void var_close(const VarState& V, VarList& L) {
  if (V.field < (uint32_t)VAL_PER_LINE) var_set(L, V.field, V.th);
}

// One byte, BEFORE sig_step of the same byte: `tok` / `dig` are S.tok / S.dig of the bytes so far.
// t: the byte's offset in the line, q: the stamp end. One fold on the token's own chain per byte:
// one more dependent 64-bit multiply next to sig_step's, as in key_step.
LP_HD void var_step(VarState& V, VarList& L, uint32_t tok, uint32_t dig, uint32_t c, int t, int q, bool on) {
  const bool dg = c - '0' < 10u;
  const bool al = dg || ((c | 32u) - 'a' < 26u);
  // a token ends on the first other byte: a field if it held a digit and is not hidden
  const bool ends = on && !al && tok != 0u && dig != 0u && V.hid == 0u;
  if (ends) var_close(V, L);
  V.field += ends ? 1u : 0u;
  if (on && al) {                       // (selects on the device: everything is in registers)
    const bool in = tok != 0u;
    V.hid = in ? V.hid : (t < q ? 1u : 0u);
    V.th = sig_fold(in ? V.th : SIG_FNV_OFFSET, c);
  }
}

// Signature and value hashes of the line text[start, start + n) (text: 16-byte aligned on the
// device): ONE forward pass, sig_step and the token state machine side by side, exactly the loads
// of line_vals_at -- aligned 16-byte loads one block ahead; never a byte before `text` or at /
// after text + tbytes. A token still open at the end of the walk -- the end of the line, or byte
// SIG_MAX_BYTES -- ends there.
LP_HD uint64_t line_vars_at(const uint8_t* __restrict__ text, int64_t tbytes, int64_t start, int n, VarList& L) {
  if (start < 0) start = 0;
  if (start > tbytes) start = tbytes;
  const int q = line_ts_span_at(text, tbytes, start, n);
  if (n > SIG_MAX_BYTES) n = SIG_MAX_BYTES;
  if ((int64_t)n > tbytes - start) n = (int)(tbytes - start);
  SigState S;
  VarState V;
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
        var_step(V, L, S.tok, S.dig, c, t, q, on);
        sig_step(S, c, on);
      }
      cur = nxt;
    }
  }
#else
  for (int t = 0; t < n; ++t) {
    var_step(V, L, S.tok, S.dig, text[start + t], t, q, true);
    sig_step(S, text[start + t], true);
  }
#endif
  if (S.tok && S.dig && !V.hid) var_close(V, L);
  return sig_finish(S);
}

}  // namespace lp
