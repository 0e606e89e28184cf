// dc_outcome.h -- launch wrappers of the game-adjudication kernels (dc_outcome.hip, dc_san.hip).
#pragma once
#include "dc_kernels.h"

namespace dc {

// dc_game_outcome (include/dchess.h) as the kernel stores it: one u64 per game,
// result | repeats << 8 | halfmove << 16 | end_ply << 32.
constexpr u32 kOutcomeBlock = 256;   // games per block, one lane each
constexpr u32 kOutcomeSlots = 151;   // half-move clocks 0..150
constexpr u32 kOutcomeKeyWords = 5;  // the four bitboards, and stm | castle | usable ep
constexpr u32 kOutcomeResults = 7;   // DC_GO_COUNT
// a block's record: validated, accepted, rejected, digest sum, digest xor, then
// the games per result
constexpr u32 kOutcomeRecord = 5 + kOutcomeResults;

// u64 words of position history for `games` lanes, laid out [slot][word][game].
inline size_t outcome_history_words(u32 games) { return (size_t)kOutcomeSlots * kOutcomeKeyWords * games; }

// One launch's batch arguments: games [first, first + count) of the batch
// (first a multiple of kOutcomeBlock) get their outcomes, digests, the bitmap's
// word columns and block records.  history holds
// outcome_history_words(hist_stride) words, hist_stride >= count.  san: ply-major
// [n_plies][n_games] SAN bytes (DC_SAN_*), 0xFF where no move was made; only
// launch_replay_san looks at it.  bitmap and digests may be null.
struct OutcomeBatch {
  const uint16_t* moves;
  u32 n_games, n_plies, first, count;
  u64* history;
  u32 hist_stride;
  u64* outcomes;
  uint8_t* san;
  u64* bitmap;
  u64* digests;
  u64* partial;
};
// The per-game arrays, in device memory: game g starts from starts[g] with clock
// min(clocks[g], 150) (null: the shared start, clock 0) and leaves the position
// it stopped in in finals[g] (null: not wanted).  All three are indexed by the
// game, whatever `first` is.
struct OutcomePerGame {
  const DevPos* starts;
  const uint16_t* clocks;
  DevPos* finals;
};

// The launchers' one argument check; start_halfmove is the shared clock (0 with
// per-game arrays).
inline bool outcome_batch_ok(const OutcomeBatch& a, u32 start_halfmove, bool want_san) {
  return a.first % kOutcomeBlock == 0 && a.count <= a.hist_stride && start_halfmove < kOutcomeSlots &&
         (u64)a.first + a.count <= a.n_games && (a.san || !want_san);
}

// Adjudicates the batch's games from `start` at clock start_halfmove
// (k_replay_outcome), or with per_game from their own starts and clocks
// (k_starts_replay_outcome, which ignores start_halfmove).
hipError_t launch_replay_outcome(hipStream_t st, const DevPos& start, u32 start_halfmove,
                                 const OutcomePerGame* per_game, const OutcomeBatch& a);
// The same plus a.san (k_replay_san, k_starts_replay_san: dc_san.hip).  Same
// history, same records.
hipError_t launch_replay_san(hipStream_t st, const DevPos& start, u32 start_halfmove, const OutcomePerGame* per_game,
                             const OutcomeBatch& a);
// totals[kOutcomeRecord] =the n_blocks block records combined (xor for the digest xor).
hipError_t launch_outcome_reduce(hipStream_t st, const u64* partial, u32 n_blocks, u64* totals);

}  // namespace dc
