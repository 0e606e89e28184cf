// dc_movegen.hip -- legal-move lists and game status for gfx950, one lane per position.
//
//   k_legal_count<G>   counts and status, block-local exclusive prefix -> offsets, block sums
//   k_legal_scan       one workgroup: 64-bit exclusive prefix of the block sums, the total
//   k_legal_emit<G,S>  every lane re-derives its moves in canonical order and
//                      writes them at its final offset (and the final offsets)
//   k_legal_fixup      the sizing call's offsets (no moves wanted)
//   k_legal_small<G,S> n <= 256: all of the above in one block, one launch
//
// The output is a dense CSR, so the lanes of a wave own adjacent ranges of the
// move array: a wave's moves are one contiguous run of u16.  The staged emit
// (S = true) collects that run in LDS, kStageChunk moves at a time, at the
// lanes' wave-prefix offsets, and streams it out as aligned dwords (an odd
// first or last u16 goes out on its own); the plain emit (S = false) stores
// each move straight from its lane.  The plain emit ships; the A/B build also
// holds the staged one (DC_LEGAL_EMIT=plain|staged).  Why plain: at 1M
// positions it took 0.51 ms against the staged one's 0.74 ms (DESIGN.md
// section 3.10) -- the kernel is bound by re-deriving the moves
// piece by piece, not by its stores, and staging adds LDS traffic, two wave
// syncs per chunk and a second enumeration for lanes that straddle chunks.
//
// No kernel waits for another block: count, scan and emit are three launches.
#include <hip/hip_runtime.h>

#include "dc_common.h"
#include "dc_movegen.h"

namespace dc {

namespace {

constexpr u32 kStageChunk = 2048;            // moves staged per wave and round (even: a run keeps its parity)
constexpr u32 kStageWave = kStageChunk + 8;  // + the parity slot, padded to 16 bytes
constexpr u32 kPosWords = kLegalBlock * 5;   // a block's positions as u64
constexpr u32 kSmemWords = (4 * kStageWave * 2 + 7) / 8 > kPosWords ? (4 * kStageWave * 2 + 7) / 8 : kPosWords;
static_assert(kStageChunk % 2 == 0 && (kStageWave * 2) % 16 == 0, "stage layout");

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
  // (from, to) ascending: ref_kth_move's order
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
template <class G, bool STAGED>
__device__ __forceinline__ void emit_wave(const LanePos& p, u32 start, u32 cnt, uint16_t* __restrict__ moves, u32 limit,
                                          uint16_t* stage /*LDS[kStageWave], this wave's*/) {
  if constexpr (!STAGED) {
    (void)stage;
    if (cnt == 0) return;
    u32 k = 0;
    auto sink = [&](u32 mv) {
      if (k < cnt && start + k < limit) moves[start + k] = (uint16_t)mv;
      ++k;
    };
    G::list(p, sink);
    while (k < cnt) sink(0xFFFFu);
  } else {
    const u32 lane = lane_id();
    const u32 w0 = lane_bcast(start, 0);
    const u32 wtot = lane_bcast(start + cnt, 63) - w0;
    if (wtot == 0) return;
    // 1 when the run starts on an odd u16 of its dword: the staged copy is
    // shifted by one slot, so staged dwords are memory dwords
    const u32 par = (u32)((reinterpret_cast<uintptr_t>(moves + w0) >> 1) & 1);
    const u32 rel = start - w0, end = rel + cnt;
    for (u32 c0 = 0; c0 < wtot; c0 += kStageChunk) {
      const u32 m = min(kStageChunk, wtot - c0);
      if (cnt != 0 && rel < c0 + m && end > c0) {  // the lane's range meets this chunk
        u32 k = rel;
        auto sink = [&](u32 mv) {
          const u32 x = k - c0;  // before the chunk: wraps past m
          if (x < m && k < end) stage[x + par] = (uint16_t)mv;
          ++k;
        };
        G::list(p, sink);
        while (k < end) sink(0xFFFFu);
      }
      wave_lds_sync();
      const u32 g0 = w0 + c0;
      if (par && lane == 0 && g0 < limit) moves[g0] = stage[1];
      const u32 body = (m - par) >> 1;  // whole dwords after the odd head
      u32* __restrict__ gd = reinterpret_cast<u32*>(moves + g0 + par);
      const u32* sd = reinterpret_cast<const u32*>(stage) + par;
      for (u32 d = lane; d < body; d += 64)
        if (g0 + par + 2 * d + 1 < limit) gd[d] = sd[d];
      if (((m - par) & 1) && lane == 0 && g0 + m - 1 < limit) moves[g0 + m - 1] = stage[m - 1 + par];
      wave_lds_sync();
    }
  }
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

template <bool STAGED>
struct LegalShared {
  alignas(16) u64 mem[STAGED ? kSmemWords : kPosWords];  // the block's positions, then the waves' stages
  u32 wsum[kLegalBlock / 64];
};

// ----------------------------------------------------------------- kernels
template <class G>
__global__ __launch_bounds__(kLegalBlock) void k_legal_count(const DevPos* __restrict__ pos, u32 n, u32* __restrict__ offsets,
                                                             uint8_t* __restrict__ status, u32* __restrict__ block_sum) {
  __shared__ LegalShared<false> sh;
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

template <class G, bool STAGED>
__global__ __launch_bounds__(kLegalBlock) void k_legal_emit(const DevPos* __restrict__ pos, u32 n, u32* offsets,
                                                            const u32* __restrict__ block_sum,
                                                            const u32* __restrict__ block_base,
                                                            uint16_t* __restrict__ moves, u32 limit) {
  __shared__ LegalShared<STAGED> sh;
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
  emit_wave<G, STAGED>(p, o + base, nx - o, moves, limit,
                       STAGED ? reinterpret_cast<uint16_t*>(sh.mem) + (tid >> 6) * kStageWave : nullptr);
}

template <class G, bool STAGED>
__global__ __launch_bounds__(kLegalBlock) void k_legal_small(const DevPos* __restrict__ pos, u32 n, u32* __restrict__ offsets,
                                                             uint8_t* __restrict__ status, uint16_t* __restrict__ moves,
                                                             u32 cap, u64* total, u32* done, u32 seq) {
  __shared__ LegalShared<STAGED> sh;
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
  if (moves && all <= cap)
    emit_wave<G, STAGED>(p, excl, cnt, moves, all, STAGED ? reinterpret_cast<uint16_t*>(sh.mem) + (tid >> 6) * kStageWave : nullptr);
  legal_publish_done(done, seq);
}

// the A/B build holds both emit variants; the product only the plain one
__host__ inline bool use_staged(bool plain) {
#ifdef DC_AB_KNOBS
  if (ab_env("DC_LEGAL_EMIT")) return !plain;
#endif
  (void)plain;
  return false;
}

}  // namespace

hipError_t launch_legal_small(hipStream_t st, u32 rules, const DevPos* pos, u32 n, u32* offsets, uint8_t* status,
                              uint16_t* moves, u32 cap, u64* total, u32* done, u32 seq, bool plain) {
  if (n == 0 || n > kLegalBlock) return hipErrorInvalidValue;
  const bool staged = use_staged(plain);
#define DC_LEGAL_SMALL(G, S) \
  hipLaunchKernelGGL((k_legal_small<G, S>), dim3(1), dim3(kLegalBlock), 0, st, pos, n, offsets, status, moves, cap, total, done, seq)
#ifdef DC_AB_KNOBS
  if (staged) {
    if (rules == 0) DC_LEGAL_SMALL(RefGen, true);
    else DC_LEGAL_SMALL(FideGen, true);
  }
#endif
  if (!staged) {
    if (rules == 0) DC_LEGAL_SMALL(RefGen, false);
    else DC_LEGAL_SMALL(FideGen, false);
  }
#undef DC_LEGAL_SMALL
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
                             const u32* block_base, uint16_t* moves, u32 limit, bool plain) {
  if (n == 0) return hipSuccess;
  const dim3 grid(blocks_for(n, kLegalBlock));
  const bool staged = use_staged(plain);
#define DC_LEGAL_EMIT(G, S) \
  hipLaunchKernelGGL((k_legal_emit<G, S>), grid, dim3(kLegalBlock), 0, st, pos, n, offsets, block_sum, block_base, moves, limit)
#ifdef DC_AB_KNOBS
  if (staged) {
    if (rules == 0) DC_LEGAL_EMIT(RefGen, true);
    else DC_LEGAL_EMIT(FideGen, true);
  }
#endif
  if (!staged) {
    if (rules == 0) DC_LEGAL_EMIT(RefGen, false);
    else DC_LEGAL_EMIT(FideGen, false);
  }
#undef DC_LEGAL_EMIT
  return hipGetLastError();
}

}  // namespace dc
