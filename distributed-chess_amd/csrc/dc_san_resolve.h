// dc_san_resolve.h -- launch wrapper of the SAN resolver kernel (dc_san_resolve.hip).
#pragma once
#include "dc_kernels.h"

namespace dc {

constexpr u32 kResolveBlock = 256;  // games per block, one lane each
constexpr u32 kResolveCounts = 5;   // DC_SR_COUNT

// Resolves the token columns of n_games games from `start` (include/dchess.h
// "notation input"): moves [n_plies][n_games] move words or flagged words,
// first_bad[n_games] (may be null), counts[kResolveCounts] (may be null; the
// kernel ADDS to it, one atomic per wave and counter: zero it first).
// per_game (k_starts_san_resolve): game g starts from starts[g] (null: `start`)
// and leaves the position after its last resolved move in finals[g] (null: not
// wanted); n_plies == 0 copies the starts.  Otherwise the two are not looked at.
hipError_t launch_san_resolve(hipStream_t st, const DevPos& start, bool per_game, const DevPos* starts, DevPos* finals,
                              const u32* tokens, u32 n_games, u32 n_plies, uint16_t* moves, u32* first_bad,
                              u64* counts);

}  // namespace dc
