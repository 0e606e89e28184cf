// dc_outcome.hip -- game adjudication under RULES_FIDE for gfx950, one lane per game.
//
//   k_replay_outcome   k_replay_fide's replay that also says where each game
//                      ended and how: checkmate, stalemate, dead position,
//                      fivefold repetition (FIDE 9.6.1), 75 moves (9.6.2)
//   k_starts_replay_outcome   the same loop (dc_outcome_lane.h, STARTS) with a start
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

#include "dc_outcome_lane.h"

namespace dc {

__global__ __launch_bounds__(kOutcomeBlock) void k_replay_outcome(Board start, u32 stm0, u32 meta0, u32 clock0,
                                                                  const uint16_t* __restrict__ moves, u32 n_games,
                                                                  u32 n_plies, u32 first, u32 count, u64* hist,
                                                                  u32 stride, u64* __restrict__ outcomes,
                                                                  u64* __restrict__ bitmap, u64* __restrict__ digests,
                                                                  u64* __restrict__ partial) {
  replay_adjudicate_lane<false, false>(start, stm0, meta0, clock0, nullptr, nullptr, nullptr, moves, n_games, n_plies,
                                       first, count, hist, stride, outcomes, nullptr, bitmap, digests, partial);
}

__global__ __launch_bounds__(kOutcomeBlock) void k_starts_replay_outcome(
    Board start, u32 stm0, u32 meta0, const DevPos* __restrict__ starts, const uint16_t* __restrict__ clocks,
    DevPos* __restrict__ finals, const uint16_t* __restrict__ moves, u32 n_games, u32 n_plies, u32 first, u32 count,
    u64* hist, u32 stride, u64* __restrict__ outcomes, u64* __restrict__ bitmap, u64* __restrict__ digests,
    u64* __restrict__ partial) {
  replay_adjudicate_lane<true, false>(start, stm0, meta0, 0, starts, clocks, finals, moves, n_games, n_plies, first,
                                      count, hist, stride, outcomes, nullptr, bitmap, digests, partial);
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

hipError_t launch_replay_outcome(hipStream_t st, const DevPos& start, u32 start_halfmove,
                                 const OutcomePerGame* per_game, const OutcomeBatch& a) {
  if (a.count == 0) return hipSuccess;
  if (!outcome_batch_ok(a, per_game ? 0 : start_halfmove, false)) return hipErrorInvalidValue;
  const dim3 grid(blocks_for(a.count, kOutcomeBlock)), block(kOutcomeBlock);
  const Board b{start.bb[0], start.bb[1], start.bb[2], start.bb[3]};
  const u32 stm = start.stm & 1, meta = pack_meta(start.castle, start.ep);
  if (per_game)
    hipLaunchKernelGGL(k_starts_replay_outcome, grid, block, 0, st, b, stm, meta, per_game->starts, per_game->clocks,
                       per_game->finals, a.moves, a.n_games, a.n_plies, a.first, a.count, a.history, a.hist_stride,
                       a.outcomes, a.bitmap, a.digests, a.partial);
  else
    hipLaunchKernelGGL(k_replay_outcome, grid, block, 0, st, b, stm, meta, start_halfmove, a.moves, a.n_games,
                       a.n_plies, a.first, a.count, a.history, a.hist_stride, a.outcomes, a.bitmap, a.digests,
                       a.partial);
  return hipGetLastError();
}

hipError_t launch_outcome_reduce(hipStream_t st, const u64* partial, u32 n_blocks, u64* totals) {
  hipLaunchKernelGGL(k_outcome_reduce, dim3(1), dim3(256), 0, st, partial, n_blocks, totals);
  return hipGetLastError();
}

}  // namespace dc
