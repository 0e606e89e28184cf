// dc_test_hash.hip -- test hook: the state hash's move-number digits on gfx950.
//
// dc_state_hash shows a move number only inside a hashed history, and the
// oracle's Python Keccak cannot hash the 2 MB start history that a seven-digit
// number needs.  dc_test_hash_digits runs the helpers k_state_hash_ref calls
// (dc_hash_digits.h: bcd_add2, bcd_emit, div_emit) for every v of a range on
// the device and counts the v where they disagree:
//   - the digits bcd_emit writes for v's packed BCD differ from the digits
//     div_emit writes for v (count or bytes), or are not v's decimal digits
//     (their value, summed back, is not v);
//   - bcd_add2(bcd(v)) != bcd(v + 2).
// bcd(v) is built here by division, as the kernel builds its first number.
// Test infrastructure only: not in include/dchess.h, not in the Rust binding.
#include "dc_ctx.h"
#include "dc_hash_digits.h"

namespace dc {
namespace {

constexpr u32 kDigitThreads = 256, kDigitBlocks = 1024;
constexpr u32 kDigitRow = 12;  // ten digits of a u32, rounded up

__device__ __forceinline__ u32 bcd_of(u32 v) {
  u32 bcd = 0;
  for (u32 sh = 0; v; v /= 10, sh += 4) bcd |= (v % 10) << sh;
  return bcd;
}

// out[0]: the number of mismatching v; out[1]: the least of them (~0: none)
__global__ __launch_bounds__(kDigitThreads) void k_test_hash_digits(u32 first, u32 count, u32* __restrict__ out) {
  // the digits go to LDS, as the kernel's token area does
  __shared__ char db[kDigitThreads][kDigitRow], dd[kDigitThreads][kDigitRow];
  char* const b = db[threadIdx.x];
  char* const d = dd[threadIdx.x];
  u32 bad = 0, least = ~0u;
  for (u32 i = blockIdx.x * kDigitThreads + threadIdx.x; i < count; i += kDigitBlocks * kDigitThreads) {
    const u32 v = first + i;
    const u32 bcd = bcd_of(v);
    const u32 nb = bcd_emit(b, bcd), nd = div_emit(d, v);
    bool ok = nb == nd && nb <= 7;
    u32 back = 0;
    for (u32 k = 0; ok && k < nb; ++k) {
      ok = b[k] == d[k] && b[k] >= '0' && b[k] <= '9';
      back = 10 * back + (u32)(b[k] - '0');
    }
    ok = ok && back == v && bcd_add2(bcd) == bcd_of(v + 2);
    if (!ok) {
      ++bad;
      least = min(least, v);
    }
  }
  if (bad) {
    atomicAdd(&out[0], bad);
    atomicMin(&out[1], least);
  }
}

}  // namespace
}  // namespace dc

// Checks every v in [first, first + count), 1 <= first and first + count <=
// 10^7 (the kernel's BCD range); out[2] on the host: mismatches, least
// mismatching v (~0 when there is none).
extern "C" __attribute__((visibility("default"))) int dc_test_hash_digits(dc_ctx* c, uint32_t first, uint32_t count,
                                                                           uint32_t* out) {
  ENTER_WORK(c);
  if (!out || first == 0 || (u64)first + count > 10000000ull) return DC_EINVAL;
  out[0] = 0;
  out[1] = ~0u;
  if (count == 0) return DC_SUCCESS;
  DBuf<u32> d_out;
  HIP_TRY(d_out.ensure(2));
  HIP_TRY(hipMemcpyAsync(d_out.p, out, 2 * sizeof(u32), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(dc::k_test_hash_digits, dim3(dc::kDigitBlocks), dim3(dc::kDigitThreads), 0, c->stream, first,
                     count, d_out.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out, d_out.p, 2 * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
  return sync_ctx(c);
}
