// dc_outcome.hip -- game adjudication under RULES_FIDE for gfx950, one lane per game.
//
//   k_replay_outcome   k_replay_fide's replay that also says where each game
//                      ended and how: checkmate, stalemate, dead position,
//                      fivefold repetition (FIDE 9.6.1), 75 moves (9.6.2)
//   k_starts_replay_outcome   the same loop (replay_outcome_lane<true>) with a start
//                      position and a clock per game, read once before ply 0,
//                      and the position each game stopped in written once after it
//   k_outcome_reduce   one workgroup: the block records -> replay counters and
//                      the result histogram
//
// Repetition needs the game's earlier positions.  A position can only recur
// inside the run of moves since the last pawn move or capture, and inside such
// a run the half-move clock numbers the positions 0, 1, 2, ...: every lane
// keeps the full key of the position at clock h (the four bitboards and one
// word of side to move, castling rights and the en-passant square where a
// capture onto it is legal) in slot h of a global history laid out
// [slot][word][game], so a wave's access to one slot is contiguous.  The
// positions the current one can equal are then exactly the slots below its
// clock, down to the clock the run began with, that share its parity (the
// same side to move); a clock reset needs no clearing, the slots above are
// simply stale.  Keys are compared whole -- the knight/king/rook/queen plane
// first, since no pawn moves inside a run, then the rest -- so a position
// counts as repeated only when it is equal: no hash, nothing to confirm.
#include <hip/hip_runtime.h>

#include "dc_common.h"
#include "dc_outcome.h"

namespace dc {

namespace {

enum : u32 { GO_ONGOING = 0, GO_WHITE_WINS, GO_BLACK_WINS, GO_STALEMATE, GO_DEAD, GO_FIVEFOLD, GO_SEVENTYFIVE };
constexpr u32 kClockEnd = kOutcomeSlots - 1;  // 150 half-moves: the 75-move rule

__device__ __forceinline__ const u64* key_at(const u64* hist, u32 slot, u32 stride, u32 lane_game) {
  return hist + (size_t)slot * kOutcomeKeyWords * stride + lane_game;
}

}  // namespace

// The adjudicating replay of one lane.  STARTS: the game's own start position
// and clock (starts / clocks, either may be null: the shared start, the shared
// clock) and, after the loop, the position it stopped in (finals, may be null);
// all three indexed by the game, not by the chunk's lane.  Otherwise the shared
// start alone, and the three pointers are not looked at.
template <bool STARTS>
__device__ __forceinline__ void replay_outcome_lane(Board start, u32 stm0, u32 meta0, u32 clock0,
                                                    const DevPos* __restrict__ starts,
                                                    const uint16_t* __restrict__ clocks, DevPos* __restrict__ finals,
                                                    const uint16_t* __restrict__ moves, u32 n_games, u32 n_plies,
                                                    u32 first, u32 count, u64* hist, u32 stride,
                                                    u64* __restrict__ outcomes, u64* __restrict__ bitmap,
                                                    u64* __restrict__ digests, u64* __restrict__ partial) {
  const u32 local = blockIdx.x * kOutcomeBlock + threadIdx.x;  // the lane's column of the history
  const u32 g = first + local;
  const bool active = local < count;
  const u32 words = (n_games + 63) >> 6;
  Board b = start;
  u32 stm = stm0, meta = meta0;
  u32 clock = clock0;  // half-move clock
  if (STARTS && active) {
    if (starts) load_start(starts, g, b, stm, meta);
    if (clocks) clock = min((u32)clocks[g], kClockEnd);  // the history has slots 0..150
  }
  u32 base = clock;  // the clock this run of reversible moves began with
  u32 result = GO_ONGOING, repeats = 1, consumed = 0, end_ply = n_plies;
  u32 validated = 0, accepted = 0;
  bool fresh = active;  // the position has not been adjudicated yet
  u32 ply = 0;
  for (;; ++ply) {
    if (fresh) {
      fresh = false;
      u64 checkers;
      const u32 n_legal = stm ? fide_count_checkers<1>(b, meta, checkers) : fide_count_checkers<0>(b, meta, checkers);
      u32 kw = (meta & 15) | (stm << 11);
      if (meta & META_EP_VALID) {
        const bool usable = stm ? fide_ep_capturable<1>(b, meta) : fide_ep_capturable<0>(b, meta);
        kw |= usable ? (meta & 0x7F0u) : 0u;
      }
      repeats = 1;
      for (int s = (int)clock - 2; s >= (int)base; s -= 2) {
        const u64* k = key_at(hist, (u32)s, stride, local);
        if (k[2 * (size_t)stride] == b.b2) {
          const bool same = k[0] == b.b0 && k[stride] == b.b1 && k[3 * (size_t)stride] == b.b3 &&
                            k[4 * (size_t)stride] == (u64)kw;
          repeats += same ? 1u : 0u;
        }
      }
      if (clock <= kClockEnd) {
        u64* k = const_cast<u64*>(key_at(hist, clock, stride, local));
        k[0] = b.b0;
        k[stride] = b.b1;
        k[2 * (size_t)stride] = b.b2;
        k[3 * (size_t)stride] = b.b3;
        k[4 * (size_t)stride] = kw;
      }
      // checkmate > stalemate > dead > fivefold > seventy-five
      result = n_legal == 0 ? (checkers ? (stm ? GO_WHITE_WINS : GO_BLACK_WINS) : GO_STALEMATE)
               : fide_insufficient(b) ? GO_DEAD
               : repeats >= 5       ? GO_FIVEFOLD
               : clock >= kClockEnd ? GO_SEVENTYFIVE
                                    : GO_ONGOING;
      if (result != GO_ONGOING) end_ply = consumed;
    }
    if (ply >= n_plies) break;
    const bool live = active && result == GO_ONGOING;
    if (ballot(live) == 0) break;  // every game of the wave has ended (a ballot is wave-uniform)
    const u32 m = live ? moves[(size_t)ply * n_games + g] : 0xFFFFu;
    bool ok = false;
    if (m != 0xFFFFu) {
      ++validated;
      ok = fide_verdict(b, stm, meta, m) == V_OK;
      if (ok) {
        const int f = (int)(m & 63), t = (int)((m >> 6) & 63);
        // a pawn move (en passant included) or a capture restarts the clock
        const bool reset = (nibble(b, f) >> 1) == KC_P || ((occupied(b) >> t) & 1);
        meta = fide_make_rt(b, stm, meta, f, t, (int)((m >> 12) & 7));
        stm ^= 1;
        ++accepted;
        clock = reset ? 0u : clock + 1;
        base = reset ? 0u : base;
        consumed = ply + 1;
        fresh = true;
      }
    }
    const u64 word = ballot(ok);
    if (bitmap && lane_id() == 0 && (g >> 6) < words) bitmap[(size_t)ply * words + (g >> 6)] = word;
  }
  // the plies no game of the wave reached: accept bits 0
  if (bitmap && ((first + (local & ~63u)) >> 6) < words) {
    const u32 w = (first + (local & ~63u)) >> 6;
    for (u32 p = ply + lane_id(); p < n_plies; p += 64) bitmap[(size_t)p * words + w] = 0;
  }
  u64 d = 0;
  if (active) {
    d = board_digest(b, stm);
    if (digests) digests[g] = d;
    outcomes[g] = (u64)result | ((u64)min(repeats, 255u) << 8) | ((u64)(clock & 0xFFFFu) << 16) | ((u64)end_ply << 32);
    if (STARTS && finals) store_final(finals, g, b, stm, meta);
  }
  // the block's record
  __shared__ u64 ws[kOutcomeBlock / 64][kOutcomeRecord];
  const u64 sv = wave_sum64(validated), sa = wave_sum64(accepted), sd = wave_sum64(d);
  u64 x = d;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x ^= __shfl_xor(x, o, 64);
  u64 by_result[kOutcomeResults];
#pragma unroll
  for (u32 k = 0; k < kOutcomeResults; ++k) by_result[k] = pc(ballot(active && result == k));
  const u32 w = threadIdx.x >> 6;
  if (lane_id() == 0) {
    ws[w][0] = sv;
    ws[w][1] = sa;
    ws[w][2] = sv - sa;
    ws[w][3] = sd;
    ws[w][4] = x;
#pragma unroll
    for (u32 k = 0; k < kOutcomeResults; ++k) ws[w][5 + k] = by_result[k];
  }
  __syncthreads();
  if (threadIdx.x < kOutcomeRecord) {
    const u32 k = threadIdx.x;
    u64 v = ws[0][k];
    for (u32 q = 1; q < kOutcomeBlock / 64; ++q) v = (k == 4) ? (v ^ ws[q][k]) : (v + ws[q][k]);
    partial[((size_t)(first / kOutcomeBlock) + blockIdx.x) * kOutcomeRecord + k] = v;
  }
}

__global__ __launch_bounds__(kOutcomeBlock) void k_replay_outcome(Board start, u32 stm0, u32 meta0, u32 clock0,
                                                                  const uint16_t* __restrict__ moves, u32 n_games,
                                                                  u32 n_plies, u32 first, u32 count, u64* hist,
                                                                  u32 stride, u64* __restrict__ outcomes,
                                                                  u64* __restrict__ bitmap, u64* __restrict__ digests,
                                                                  u64* __restrict__ partial) {
  replay_outcome_lane<false>(start, stm0, meta0, clock0, nullptr, nullptr, nullptr, moves, n_games, n_plies, first,
                             count, hist, stride, outcomes, bitmap, digests, partial);
}

__global__ __launch_bounds__(kOutcomeBlock) void k_starts_replay_outcome(
    Board start, u32 stm0, u32 meta0, const DevPos* __restrict__ starts, const uint16_t* __restrict__ clocks,
    DevPos* __restrict__ finals, const uint16_t* __restrict__ moves, u32 n_games, u32 n_plies, u32 first, u32 count,
    u64* hist, u32 stride, u64* __restrict__ outcomes, u64* __restrict__ bitmap, u64* __restrict__ digests,
    u64* __restrict__ partial) {
  replay_outcome_lane<true>(start, stm0, meta0, 0, starts, clocks, finals, moves, n_games, n_plies, first, count, hist,
                            stride, outcomes, bitmap, digests, partial);
}

__global__ __launch_bounds__(256) void k_outcome_reduce(const u64* __restrict__ partial, u32 n_blocks,
                                                        u64* __restrict__ totals) {
  __shared__ u64 ws[4][kOutcomeRecord];
  for (u32 k = 0; k < kOutcomeRecord; ++k) {
    u64 r = 0;
    for (u32 blk = threadIdx.x; blk < n_blocks; blk += blockDim.x) {
      const u64 v = partial[(size_t)blk * kOutcomeRecord + k];
      r = (k == 4) ? (r ^ v) : (r + v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const u64 y = __shfl_xor(r, o, 64);
      r = (k == 4) ? (r ^ y) : (r + y);
    }
    if (lane_id() == 0) ws[threadIdx.x >> 6][k] = r;
  }
  __syncthreads();
  if (threadIdx.x < kOutcomeRecord) {
    const u32 k = threadIdx.x;
    u64 v = ws[0][k];
    for (u32 q = 1; q < 4; ++q) v = (k == 4) ? (v ^ ws[q][k]) : (v + ws[q][k]);
    totals[k] = v;
  }
}

hipError_t launch_replay_outcome(hipStream_t st, const DevPos& start, u32 start_halfmove, const uint16_t* moves,
                                 u32 n_games, u32 n_plies, u32 first, u32 count, u64* history, u32 hist_stride,
                                 u64* outcomes, u64* bitmap, u64* digests, u64* partial) {
  if (count == 0) return hipSuccess;
  if (first % kOutcomeBlock != 0 || count > hist_stride || start_halfmove >= kOutcomeSlots ||
      (u64)first + count > n_games)
    return hipErrorInvalidValue;
  const Board b{start.bb[0], start.bb[1], start.bb[2], start.bb[3]};
  hipLaunchKernelGGL(k_replay_outcome, dim3(blocks_for(count, kOutcomeBlock)), dim3(kOutcomeBlock), 0, st, b,
                     (u32)(start.stm & 1), (u32)pack_meta(start.castle, start.ep), start_halfmove, moves, n_games,
                     n_plies, first, count, history, hist_stride, outcomes, bitmap, digests, partial);
  return hipGetLastError();
}

hipError_t launch_replay_outcome_starts(hipStream_t st, const DevPos* starts, const uint16_t* start_halfmoves,
                                        DevPos* finals, const uint16_t* moves, u32 n_games, u32 n_plies, u32 first,
                                        u32 count, u64* history, u32 hist_stride, u64* outcomes, u64* bitmap,
                                        u64* digests, u64* partial) {
  if (count == 0) return hipSuccess;
  if (first % kOutcomeBlock != 0 || count > hist_stride || (u64)first + count > n_games) return hipErrorInvalidValue;
  Board b;
  startpos_board(b);
  hipLaunchKernelGGL(k_starts_replay_outcome, dim3(blocks_for(count, kOutcomeBlock)), dim3(kOutcomeBlock), 0, st, b,
                     0u, (u32)pack_meta(15, -1), starts, start_halfmoves, finals, moves, n_games, n_plies, first,
                     count, history, hist_stride, outcomes, bitmap, digests, partial);
  return hipGetLastError();
}

hipError_t launch_outcome_reduce(hipStream_t st, const u64* partial, u32 n_blocks, u64* totals) {
  hipLaunchKernelGGL(k_outcome_reduce, dim3(1), dim3(256), 0, st, partial, n_blocks, totals);
  return hipGetLastError();
}

}  // namespace dc
