// dc_san.hip -- k_replay_outcome's adjudicating replay (dc_outcome.hip) that also
// says what was played: one SAN byte per accepted ply (include/dchess.h DC_SAN_*).
//
//   k_replay_san   one lane per game; the loop (dc_outcome_lane.h, SAN), the
//                  position history, the chunking and the block records are
//                  k_replay_outcome's (k_outcome_reduce combines the records
//                  of either)
//   k_starts_replay_san   the same lane body (STARTS) with
//                  k_starts_replay_outcome's per-game starts, clocks and finals
//
// The byte of ply p has two halves.  Kind, capture and the disambiguation
// flags are known when the move is validated: the validation's own analysis
// (pins, checkers) decides which other pieces of the mover's kind could legally
// go to the same square.  Check and mate are the child's adjudication, which
// the loop does anyway one iteration later (checkers != 0, n_legal == 0): the
// lane keeps the first half until then, and every trip of the loop stores the
// byte of the ply before it (0xFF where that ply made no move).  No second move
// generation, one byte store per ply.
#include <hip/hip_runtime.h>

#include "dc_outcome_lane.h"

namespace dc {

__global__ __launch_bounds__(kOutcomeBlock) void k_replay_san(Board start, u32 stm0, u32 meta0, u32 clock0,
                                                              const uint16_t* __restrict__ moves, u32 n_games,
                                                              u32 n_plies, u32 first, u32 count, u64* hist, u32 stride,
                                                              u64* __restrict__ outcomes, uint8_t* __restrict__ san,
                                                              u64* __restrict__ bitmap, u64* __restrict__ digests,
                                                              u64* __restrict__ partial) {
  replay_adjudicate_lane<false, true>(start, stm0, meta0, clock0, nullptr, nullptr, nullptr, moves, n_games, n_plies,
                                      first, count, hist, stride, outcomes, san, bitmap, digests, partial);
}

__global__ __launch_bounds__(kOutcomeBlock) void k_starts_replay_san(
    Board start, u32 stm0, u32 meta0, const DevPos* __restrict__ starts, const uint16_t* __restrict__ clocks,
    DevPos* __restrict__ finals, const uint16_t* __restrict__ moves, u32 n_games, u32 n_plies, u32 first, u32 count,
    u64* hist, u32 stride, u64* __restrict__ outcomes, uint8_t* __restrict__ san, u64* __restrict__ bitmap,
    u64* __restrict__ digests, u64* __restrict__ partial) {
  replay_adjudicate_lane<true, true>(start, stm0, meta0, 0, starts, clocks, finals, moves, n_games, n_plies, first,
                                     count, hist, stride, outcomes, san, bitmap, digests, partial);
}

hipError_t launch_replay_san(hipStream_t st, const DevPos& start, u32 start_halfmove, const OutcomePerGame* per_game,
                             const OutcomeBatch& a) {
  if (a.count == 0) return hipSuccess;
  if (!outcome_batch_ok(a, per_game ? 0 : start_halfmove, true)) return hipErrorInvalidValue;
  const dim3 grid(blocks_for(a.count, kOutcomeBlock)), block(kOutcomeBlock);
  const Board b{start.bb[0], start.bb[1], start.bb[2], start.bb[3]};
  const u32 stm = start.stm & 1, meta = pack_meta(start.castle, start.ep);
  if (per_game)
    hipLaunchKernelGGL(k_starts_replay_san, grid, block, 0, st, b, stm, meta, per_game->starts, per_game->clocks,
                       per_game->finals, a.moves, a.n_games, a.n_plies, a.first, a.count, a.history, a.hist_stride,
                       a.outcomes, a.san, a.bitmap, a.digests, a.partial);
  else
    hipLaunchKernelGGL(k_replay_san, grid, block, 0, st, b, stm, meta, start_halfmove, a.moves, a.n_games, a.n_plies,
                       a.first, a.count, a.history, a.hist_stride, a.outcomes, a.san, a.bitmap, a.digests, a.partial);
  return hipGetLastError();
}

}  // namespace dc
