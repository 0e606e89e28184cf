// dc_test_secp.hip -- test hook: one secp256k1 operation per lane on gfx950.
//
// dc_verify_tx_batch shows only a verdict, and an honestly signed transaction
// cannot steer the operands of the arithmetic below it.  dc_test_secp_op runs
// one dc_secp.h operation per record on the device -- the Comba / inline-asm
// branch of mul_wide, sqr_wide, fe_reduce and sc_fold that the host unit test
// (tests/cpp/test_secp.cpp) never compiles -- and hands the result back, so
// tests/test_secp_device.py can compare it with Python big integers.  Test
// infrastructure only: not in include/dchess.h, not in the Rust binding.
//
// A record is five 256-bit operands (8 little-endian u32 limbs each, 40 words)
// in and two 256-bit results plus a flag word (17 words) out.  Operands are
// reduced (mod p or mod n, as the operation reads them) on entry.
//
//   op  name        operands           results            flag
//    0  fe_mul      a, b               a b mod p
//    1  fe_sqr      a                  a^2 mod p
//    2  fe_add      a, b               a + b mod p
//    3  fe_sub      a, b               a - b mod p
//    4  fe_inv      a                  a^(p-2) mod p
//    5  fe_sqrt     a                  a^((p+1)/4) mod p  1 iff its square is a
//    6  sc_mul      a, b               a b mod n
//    7  sc_inv      a                  a^(n-2) mod n
//    8  sc_add      a, b               a + b mod n
//    9  split       k                  k1, k2 (mod n)     k = k1 + lambda k2
//   10  ecmult      u1, u2, Qx, Qy     x, y of u1 G + u2 Q  1 iff infinity
//   11  verify_raw  z, r, s, Qx, Qy                       1 iff ecdsa_verify accepts
//   12  gtab        k (limb 0)         x, y of the context's G-table entry k
// Ops 10 and 11 set the flag to ~0 when Q is not on the curve, op 12 when
// k is not a table index; nothing is computed then.
#include "dc_ctx.h"
#include "dc_txsig.h"
#include "dc_txsig_k.h"

namespace dc {
namespace {

constexpr u32 kProbeIn = 40, kProbeOut = 17, kProbeOps = 13;
constexpr u32 kProbeThreads = 128;  // k_verify_tx's launch bounds: ops 10 and 11 run its ecmult

__device__ __forceinline__ void copy8(u32 (&r)[8], const u32 (&a)[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) r[k] = a[k];
}

template <int OP>
__global__ __launch_bounds__(kProbeThreads, 2) void k_test_secp(const u32* __restrict__ in, u32 n,
                                                                 const secp::Ge* __restrict__ gtab,
                                                                 u32* __restrict__ out) {
  using namespace secp;
  const u32 i = blockIdx.x * kProbeThreads + threadIdx.x;
  if (i >= n) return;
  const u32* p = in + (size_t)kProbeIn * i;
  u32 a[8], b[8], c[8], d[8], e[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    a[k] = p[k];
    b[k] = p[8 + k];
    c[k] = p[16 + k];
    d[k] = p[24 + k];
    e[k] = p[32 + k];
  }
  u32 r0[8], r1[8], flag = 0;
  set_zero(r0);
  set_zero(r1);
  if constexpr (OP <= 5) {
    Fe x, y, r;
    fe_canon(x, a);
    fe_canon(y, b);
    if constexpr (OP == 0) fe_mul(r, x, y);
    if constexpr (OP == 1) fe_sqr(r, x);
    if constexpr (OP == 2) fe_add(r, x, y);
    if constexpr (OP == 3) fe_sub(r, x, y);
    if constexpr (OP == 4) fe_inv(r, x);
    if constexpr (OP == 5) {
      fe_pow_sqrt(r, x);
      Fe q;
      fe_sqr(q, r);
      flag = eq8(q.v, x.v) ? 1u : 0u;
    }
    copy8(r0, r.v);
  } else if constexpr (OP <= 8) {
    Sc x, y, r;
    sc_canon(x, a);
    sc_canon(y, b);
    if constexpr (OP == 6) sc_mul(r, x, y);
    if constexpr (OP == 7) sc_inv(r, x);
    if constexpr (OP == 8) sc_add(r, x, y);
    copy8(r0, r.v);
  } else if constexpr (OP == 9) {
    Sc k, k1, k2;
    sc_canon(k, a);
    sc_split_lambda(k1, k2, k);
    copy8(r0, k1.v);
    copy8(r1, k2.v);
  } else if constexpr (OP == 10) {
    Sc u1, u2;
    Ge q;
    sc_canon(u1, a);
    sc_canon(u2, b);
    fe_canon(q.x, c);
    fe_canon(q.y, d);
    if (!ge_on_curve(q)) {
      flag = ~0u;
    } else {
      Gej R;
      ecmult(R, q, u2, u1, gtab);
      if (R.inf) {
        flag = 1;
      } else {
        Ge t;
        gej_to_ge(t, R);
        copy8(r0, t.x.v);
        copy8(r1, t.y.v);
      }
    }
  } else if constexpr (OP == 11) {
    Sc z, r, s;
    Ge q;
    sc_canon(z, a);
    sc_canon(r, b);
    sc_canon(s, c);
    fe_canon(q.x, d);
    fe_canon(q.y, e);
    if (!ge_on_curve(q)) flag = ~0u;
    else flag = ecdsa_verify(r, s, z, q, gtab) ? 1u : 0u;
  } else {
    if (a[0] >= (u32)kGTabEntries) {
      flag = ~0u;
    } else {
      const Ge g = gtab[a[0]];
      copy8(r0, g.x.v);
      copy8(r1, g.y.v);
    }
  }
  u32* o = out + (size_t)kProbeOut * i;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    o[k] = r0[k];
    o[8 + k] = r1[k];
  }
  o[16] = flag;
}

template <int OP>
hipError_t launch_test_secp(hipStream_t st, const u32* in, u32 n, const secp::Ge* gtab, u32* out) {
  hipLaunchKernelGGL(k_test_secp<OP>, dim3((n + kProbeThreads - 1) / kProbeThreads), dim3(kProbeThreads), 0, st, in, n,
                     gtab, out);
  return hipGetLastError();
}

hipError_t launch_test_secp_op(u32 op, hipStream_t st, const u32* in, u32 n, const secp::Ge* gtab, u32* out) {
  switch (op) {
    case 0: return launch_test_secp<0>(st, in, n, gtab, out);
    case 1: return launch_test_secp<1>(st, in, n, gtab, out);
    case 2: return launch_test_secp<2>(st, in, n, gtab, out);
    case 3: return launch_test_secp<3>(st, in, n, gtab, out);
    case 4: return launch_test_secp<4>(st, in, n, gtab, out);
    case 5: return launch_test_secp<5>(st, in, n, gtab, out);
    case 6: return launch_test_secp<6>(st, in, n, gtab, out);
    case 7: return launch_test_secp<7>(st, in, n, gtab, out);
    case 8: return launch_test_secp<8>(st, in, n, gtab, out);
    case 9: return launch_test_secp<9>(st, in, n, gtab, out);
    case 10: return launch_test_secp<10>(st, in, n, gtab, out);
    case 11: return launch_test_secp<11>(st, in, n, gtab, out);
    default: return launch_test_secp<12>(st, in, n, gtab, out);
  }
}

}  // namespace
}  // namespace dc

// in: n records of 40 words, out: n records of 17 words, both host buffers.
extern "C" __attribute__((visibility("default"))) int dc_test_secp_op(dc_ctx* c, uint32_t op, const uint32_t* in,
                                                                       uint32_t n, uint32_t* out) {
  ENTER_WORK(c);
  if (op >= dc::kProbeOps) return DC_EINVAL;
  if (n == 0) return DC_SUCCESS;
  if (!in || !out) return DC_EINVAL;
  const int e = ensure_gtab(c);
  if (e != DC_SUCCESS) return e;
  DBuf<u32> d_in, d_out;
  HIP_TRY(d_in.ensure((size_t)dc::kProbeIn * n));
  HIP_TRY(d_out.ensure((size_t)dc::kProbeOut * n));
  HIP_TRY(hipMemcpyAsync(d_in.p, in, (size_t)dc::kProbeIn * n * sizeof(u32), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(dc::launch_test_secp_op(op, c->stream, d_in.p, n, c->gtab.p, d_out.p));
  HIP_TRY(hipMemcpyAsync(out, d_out.p, (size_t)dc::kProbeOut * n * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
  return sync_ctx(c);
}
