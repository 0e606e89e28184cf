// dc_hash_digits.h -- the move numbers of k_state_hash_ref's history tokens.
//
// A history token is "N. san" with N = 1 + the whitespace tokens before it
// (chess.rs:169-183), so N grows by 2 per accepted move.  While every number
// of a batch stays below 10^7 the kernel keeps N as 32-bit packed BCD (one
// decimal digit per nibble) and advances it with a BCD add; else it divides.
// The add and the two digit emissions live here so that the test hook of
// dc_test_hash.hip runs the very code the kernel runs.
#pragma once
#include "dc_common.h"

namespace dc {

// a + 2 on 32-bit packed BCD (7 digits: callers keep the numbers below 10^7)
__device__ __forceinline__ u32 bcd_add2(u32 a) {
  const u32 t1 = a + 0x06666666u, t2 = t1 + 2, t3 = t1 ^ 2;
  const u32 t5 = ~(t2 ^ t3) & 0x11111110u;  // the digits that carried
  return t2 - ((t5 >> 2) | (t5 >> 3));
}

// The decimal digits of a packed-BCD number into d, first digit first;
// returns their count.  (Round 4 built them in a dynamically indexed register
// array: 29 % of the kernel's issue cycles in tools/bbprof.py's count.)
__device__ __forceinline__ u32 bcd_emit(char* d, u32 bcd) {
  const u32 nd = max(1u, (35u - (u32)__clz((int)bcd)) >> 2);
  for (u32 i = 0; i < nd; ++i) d[i] = (char)('0' + __builtin_amdgcn_ubfe(bcd, 4 * (nd - 1 - i), 4));
  return nd;
}

// The decimal digits of v into d by division (written last-first); returns
// their count.
__device__ __forceinline__ u32 div_emit(char* d, u32 v) {
  u32 nd = 1;
  for (u32 q = v; q >= 10; q /= 10) ++nd;
  for (u32 i = nd; i-- > 0;) {
    d[i] = (char)('0' + v % 10);
    v /= 10;
  }
  return nd;
}

}  // namespace dc
