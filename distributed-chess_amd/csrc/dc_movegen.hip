// dc_movegen.hip -- legal-move lists and game status for gfx950, one lane per position.
//
//   k_legal_count<G>   counts and status, block-local exclusive prefix -> offsets, block sums
//   k_legal_scan       one workgroup: 64-bit exclusive prefix of the block sums, the total
//   k_legal_emit<G>    every lane re-derives its moves in canonical order and
//                      writes them at its final offset (and the final offsets)
//   k_legal_fixup      the sizing call's offsets (no moves wanted)
//   k_legal_small<G>   n <= 256: all of the above in one block, one launch
//
// The output is a dense CSR, so the lanes of a wave own adjacent ranges of the
// move array; each move is stored straight from its lane.  (An emit that staged
// a wave's run in LDS and streamed it out as aligned dwords took 0.74 ms at 1M
// positions against 0.51 ms and was removed, DESIGN.md section 3.10: the kernel
// is bound by re-deriving the moves piece by piece, not by its stores.)
//
// No kernel waits for another block: count, scan and emit are three launches.
#include <hip/hip_runtime.h>

#include "dc_common.h"
#include "dc_movegen.h"

namespace dc {

namespace {

constexpr u32 kPosWords = kLegalBlock * 5;  // a block's positions as u64

struct LanePos {
  Board b;
  u32 stm, meta;
};

// A block's positions through LDS: consecutive lanes load consecutive u64 of
// the 40-byte records (512 contiguous bytes per wave instruction), then every
// lane picks its five words (stride 10 dwords: conflict-free ds_read_b64).
// Ends with a barrier, so the caller may reuse smem.
__device__ __forceinline__ LanePos load_block_pos(const DevPos* __restrict__ pos, u32 first, u32 n, u64* smem,
                                                  bool fide) {
  const u32 tid = threadIdx.x;
  const u32 here = min(kLegalBlock, n - first);
  const u64* __restrict__ src = reinterpret_cast<const u64*>(pos + first);
  for (u32 k = tid; k < here * 5; k += kLegalBlock) smem[k] = src[k];
  __syncthreads();
  LanePos p{Board{0, 0, 0, 0}, 0, 0};
  if (tid < here) {
    p.b = Board{smem[5 * tid], smem[5 * tid + 1], smem[5 * tid + 2], smem[5 * tid + 3]};
    const u32 w = (u32)smem[5 * tid + 4];  // stm | castle << 8 | ep << 16
    p.stm = w & 1;
    p.meta = fide ? pack_meta((uint8_t)(w >> 8), (int8_t)(w >> 16)) : 0u;
  }
  __syncthreads();
  return p;
}

// ------------------------------------------------------------------ rules
struct RefGen {
  static constexpr bool kFide = false;
  static __device__ __forceinline__ u32 count(const LanePos& p) { return ref_count_rt(p.b, p.stm); }
  static __device__ __forceinline__ u32 status(const LanePos&) { return 0; }  // kings are capturable: no check, no dead
  // (from, to) ascending: the REF game generator's order
  template <class Sink>
  static __device__ __forceinline__ void list(const LanePos& p, Sink&& sink) {
    const u64 occ = occupied(p.b);
    u64 own = p.stm ? p.b.b0 : (occ & ~p.b.b0);
    while (own) {
      const int f = lsb(own);
      own &= own - 1;
      u64 t = ref_piece_targets(p.b, f, p.stm, nibble(p.b, f) >> 1);
      while (t) {
        const int to = lsb(t);
        t &= t - 1;
        sink((u32)f | ((u32)to << 6));
      }
    }
  }
};

template <int STM>
__device__ __forceinline__ u32 fide_in_check(const Board& b) {
  const FPos<STM> f = fpos<STM>(b);
  // what Analysis::checkers holds, without the attack map: the pieces that
  // attack our king (pawns, knights, the first piece on each line)
  const int ksq = lsb(f.K | (1ull << 63)) & 63;
  const u64 k = f.K & (1ull << ksq);  // no king: empty
  const Lines l = lines_of(ksq);
  const u64 orth = line_attacks(ksq, l.file, f.occ) | line_attacks(ksq, l.rank, f.occ);
  const u64 diag = line_attacks(ksq, l.diag, f.occ) | line_attacks(ksq, l.anti, f.occ);
  const u64 att = (pawn_attacks<STM>(k) & f.tP) | (knight_attacks(k) & f.tN) | (orth & f.tO) | (diag & f.tD);
  return (k != 0 && att != 0) ? (u32)ST_CHECK : 0u;
}

// DC_ST_DEAD: insufficient material (dc_fide_rules.h fide_insufficient).
__device__ __forceinline__ u32 fide_dead(const Board& b) { return fide_insufficient(b) ? (u32)ST_DEAD : 0u; }

template <int STM, class Sink>
__device__ __forceinline__ void fide_list_stm(const Board& b, u32 meta, Sink&& sink) {
  typedef FDir<STM> FD;
  const FPos<STM> f = fpos<STM>(b);
  const Analysis a = analyse<STM>(f);
  u64 own = f.us;
  while (own) {
    const int s = lsb(own);
    own &= own - 1;
    u64 t = fide_piece_targets<STM>(b, meta, f, a, s);
    // a pawn's targets on the last row are promotions: N, B, R, Q
    const u64 promo = ((1ull << s) & f.P) ? FD::LAST : 0ull;
    while (t) {
      const int to = lsb(t);
      t &= t - 1;
      const u32 m = (u32)s | ((u32)to << 6);
      if ((promo >> to) & 1) {
#pragma unroll
        for (u32 pr = 1; pr <= 4; ++pr) sink(m | (pr << 12));
      } else {
        sink(m);
      }
    }
  }
}

struct FideGen {
  static constexpr bool kFide = true;
  static __device__ __forceinline__ u32 count(const LanePos& p) { return fide_count_rt(p.b, p.stm, p.meta); }
  static __device__ __forceinline__ u32 status(const LanePos& p) {
    return (p.stm ? fide_in_check<1>(p.b) : fide_in_check<0>(p.b)) | fide_dead(p.b);
  }
  // (from, to, promo) ascending: fide_kth_move's order
  template <class Sink>
  static __device__ __forceinline__ void list(const LanePos& p, Sink&& sink) {
    if (p.stm) fide_list_stm<1>(p.b, p.meta, sink);
    else fide_list_stm<0>(p.b, p.meta, sink);
  }
};

// ------------------------------------------------------------------- scans
// Exclusive prefix of v over the block's 256 lanes (DPP inside the wave, the
// four wave totals through LDS); *total = the block's sum.
__device__ __forceinline__ u32 block_excl_scan(u32 v, u32* wsum /*LDS[4]*/, u32* total) {
  const u32 incl = wave_incl_scan(v);
  const u32 w = threadIdx.x >> 6;
  if (lane_id() == 63) wsum[w] = incl;
  __syncthreads();
  u32 before = 0, all = 0;
#pragma unroll
  for (u32 k = 0; k < kLegalBlock / 64; ++k) {
    const u32 x = wsum[k];
    before += k < w ? x : 0u;
    all += x;
  }
  __syncthreads();
  *total = all;
  return before + incl - v;
}

// -------------------------------------------------------------------- emit
// The moves of one wave.  start = the lane's first index in `moves`, cnt = its
// count (0 for a lane without a position); the lanes' ranges are adjacent and
// ascending.  The enumeration is cut at cnt and padded with DC_MOVE_NONE should
// it come short (count and enumeration agree on every position with at most
// one king per side), so a lane never leaves its own range.
template <class G>
__device__ __forceinline__ void emit_wave(const LanePos& p, u32 start, u32 cnt, uint16_t* __restrict__ moves, u32 limit) {
  if (cnt == 0) return;
  u32 k = 0;
  auto sink = [&](u32 mv) {
    if (k < cnt && start + k < limit) moves[start + k] = (uint16_t)mv;
    ++k;
  };
  G::list(p, sink);
  while (k < cnt) sink(0xFFFFu);
}

// Completion flag of a one-block launch whose outputs are pinned host memory
// (dc_moves.hip publish_done): every thread's stores at system scope, then
// the flag.
__device__ __forceinline__ void legal_publish_done(u32* done, u32 seq) {
  if (!done) return;
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) {
    __hip_atomic_store(done, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

struct LegalShared {
  alignas(16) u64 mem[kPosWords];  // the block's positions
  u32 wsum[kLegalBlock / 64];
};

// ----------------------------------------------------------------- kernels
template <class G>
__global__ __launch_bounds__(kLegalBlock) void k_legal_count(const DevPos* __restrict__ pos, u32 n, u32* __restrict__ offsets,
                                                             uint8_t* __restrict__ status, u32* __restrict__ block_sum) {
  __shared__ LegalShared sh;
  const u32 first = blockIdx.x * kLegalBlock, i = first + threadIdx.x;
  const bool active = i < n;
  const LanePos p = load_block_pos(pos, first, n, sh.mem, G::kFide);
  u32 cnt = 0;
  if (active) {
    cnt = G::count(p);
    if (status) status[i] = (uint8_t)(G::status(p) | (cnt == 0 ? (u32)ST_NO_MOVES : 0u));
  }
  u32 all;
  const u32 excl = block_excl_scan(cnt, sh.wsum, &all);
  if (active) offsets[i] = excl;
  if (threadIdx.x == 0) block_sum[blockIdx.x] = all;
}

__global__ __launch_bounds__(kLegalBlock) void k_legal_scan(const u32* __restrict__ block_sum, u32 n_blocks,
                                                            u32* __restrict__ block_base, u32* __restrict__ offsets_n,
                                                            u64* total) {
  __shared__ u64 wsum[kLegalBlock / 64];
  const u32 per = (n_blocks + kLegalBlock - 1) / kLegalBlock;
  const u64 a64 = (u64)threadIdx.x * per;
  const u32 a = a64 < n_blocks ? (u32)a64 : n_blocks, b = (n_blocks - a) < per ? n_blocks : a + per;
  u64 s = 0;
  for (u32 c = a; c < b; ++c) s += block_sum[c];
  const u64 incl = wave_incl_scan64(s);
  const u32 w = threadIdx.x >> 6;
  if (lane_id() == 63) wsum[w] = incl;
  __syncthreads();
  u64 before = 0, all = 0;
#pragma unroll
  for (u32 k = 0; k < kLegalBlock / 64; ++k) {
    const u64 x = wsum[k];
    before += k < w ? x : 0ull;
    all += x;
  }
  u64 run = before + incl - s;
  for (u32 c = a; c < b; ++c) {
    block_base[c] = (u32)run;  // meaningful only when the total fits 32 bits (the caller checks)
    run += block_sum[c];
  }
  if (threadIdx.x == 0) {
    *offsets_n = (u32)all;
    __hip_atomic_store(total, all, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);  // pinned host memory
  }
}

__global__ __launch_bounds__(kLegalBlock) void k_legal_fixup(u32* __restrict__ offsets, u32 n,
                                                             const u32* __restrict__ block_base) {
  const u32 i = blockIdx.x * kLegalBlock + threadIdx.x;
  if (i < n) offsets[i] += block_base[blockIdx.x];
}

template <class G>
__global__ __launch_bounds__(kLegalBlock) void k_legal_emit(const DevPos* __restrict__ pos, u32 n, u32* offsets,
                                                            const u32* __restrict__ block_sum,
                                                            const u32* __restrict__ block_base,
                                                            uint16_t* __restrict__ moves, u32 limit) {
  __shared__ LegalShared sh;
  const u32 tid = threadIdx.x, first = blockIdx.x * kLegalBlock, i = first + tid;
  const bool active = i < n;
  const LanePos p = load_block_pos(pos, first, n, sh.mem, G::kFide);
  // the lane's count from the block-local prefix k_legal_count left (the next
  // lane's, or the block's sum), read by all before any lane makes its own final
  const u32 bsum = block_sum[blockIdx.x], base = block_base[blockIdx.x];
  u32 o = bsum, nx = bsum;
  if (active) {
    o = offsets[i];
    if (tid + 1 < kLegalBlock && i + 1 < n) nx = offsets[i + 1];
  }
  __syncthreads();
  if (active) offsets[i] = o + base;
  emit_wave<G>(p, o + base, nx - o, moves, limit);
}

template <class G>
__global__ __launch_bounds__(kLegalBlock) void k_legal_small(const DevPos* __restrict__ pos, u32 n, u32* __restrict__ offsets,
                                                             uint8_t* __restrict__ status, uint16_t* __restrict__ moves,
                                                             u32 cap, u64* total, u32* done, u32 seq) {
  __shared__ LegalShared sh;
  const u32 tid = threadIdx.x;
  const bool active = tid < n;
  const LanePos p = load_block_pos(pos, 0, n, sh.mem, G::kFide);
  u32 cnt = 0;
  if (active) {
    cnt = G::count(p);
    if (status) status[tid] = (uint8_t)(G::status(p) | (cnt == 0 ? (u32)ST_NO_MOVES : 0u));
  }
  u32 all;
  const u32 excl = block_excl_scan(cnt, sh.wsum, &all);
  if (active) offsets[tid] = excl;
  if (tid == 0) {
    offsets[n] = all;
    __hip_atomic_store(total, (u64)all, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  if (moves && all <= cap) emit_wave<G>(p, excl, cnt, moves, all);
  legal_publish_done(done, seq);
}

}  // namespace

hipError_t launch_legal_small(hipStream_t st, u32 rules, const DevPos* pos, u32 n, u32* offsets, uint8_t* status,
                              uint16_t* moves, u32 cap, u64* total, u32* done, u32 seq) {
  if (n == 0 || n > kLegalBlock) return hipErrorInvalidValue;
  if (rules == 0)
    hipLaunchKernelGGL(k_legal_small<RefGen>, dim3(1), dim3(kLegalBlock), 0, st, pos, n, offsets, status, moves, cap,
                       total, done, seq);
  else
    hipLaunchKernelGGL(k_legal_small<FideGen>, dim3(1), dim3(kLegalBlock), 0, st, pos, n, offsets, status, moves, cap,
                       total, done, seq);
  return hipGetLastError();
}

hipError_t launch_legal_count(hipStream_t st, u32 rules, const DevPos* pos, u32 n, u32* offsets, uint8_t* status,
                              u32* block_sum) {
  if (n == 0) return hipSuccess;
  const dim3 grid(blocks_for(n, kLegalBlock));
  if (rules == 0)
    hipLaunchKernelGGL(k_legal_count<RefGen>, grid, dim3(kLegalBlock), 0, st, pos, n, offsets, status, block_sum);
  else
    hipLaunchKernelGGL(k_legal_count<FideGen>, grid, dim3(kLegalBlock), 0, st, pos, n, offsets, status, block_sum);
  return hipGetLastError();
}

hipError_t launch_legal_scan(hipStream_t st, const u32* block_sum, u32 n_blocks, u32* block_base, u32* offsets_n,
                             u64* total) {
  hipLaunchKernelGGL(k_legal_scan, dim3(1), dim3(kLegalBlock), 0, st, block_sum, n_blocks, block_base, offsets_n, total);
  return hipGetLastError();
}

hipError_t launch_legal_fixup(hipStream_t st, u32* offsets, u32 n, const u32* block_base) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_legal_fixup, dim3(blocks_for(n, kLegalBlock)), dim3(kLegalBlock), 0, st, offsets, n, block_base);
  return hipGetLastError();
}

hipError_t launch_legal_emit(hipStream_t st, u32 rules, const DevPos* pos, u32 n, u32* offsets, const u32* block_sum,
                             const u32* block_base, uint16_t* moves, u32 limit) {
  if (n == 0) return hipSuccess;
  const dim3 grid(blocks_for(n, kLegalBlock));
  if (rules == 0)
    hipLaunchKernelGGL(k_legal_emit<RefGen>, grid, dim3(kLegalBlock), 0, st, pos, n, offsets, block_sum, block_base,
                       moves, limit);
  else
    hipLaunchKernelGGL(k_legal_emit<FideGen>, grid, dim3(kLegalBlock), 0, st, pos, n, offsets, block_sum, block_base,
                       moves, limit);
  return hipGetLastError();
}

}  // namespace dc
