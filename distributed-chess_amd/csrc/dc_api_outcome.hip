// dc_api_outcome.hip -- game adjudication (dc_replay_outcome*, dc_replay_san*) and the FEN clocks.
#include <cstring>

#include "dc_ctx.h"
#include "dc_outcome.h"

namespace {

// The batch is adjudicated in chunks of at most this many games, so the
// position history (6040 bytes a game) stays bounded whatever n_games is.
u32 chunk_games(const dc_ctx* c) {
  const u32 k = c->outcome_chunk_games / dc::kOutcomeBlock * dc::kOutcomeBlock;
  return std::max<u32>(k, dc::kOutcomeBlock);
}

// The per-game arrays of the *_starts calls, in device memory (each may be null).
struct PerGame {
  const DevPos* starts;
  const uint16_t* clocks;
  DevPos* finals;
};

// d_san == nullptr: k_replay_outcome; else k_replay_san, which also fills d_san.
// per_game != nullptr: the *_starts kernels instead, which ignore start and
// start_halfmove.
int outcome_impl(dc_ctx* c, const dc_pos* start, uint32_t start_halfmove, const uint16_t* d_moves, uint32_t n_games,
                 uint32_t n_plies, u64* d_outcomes, uint8_t* d_san, u64* d_bitmap, u64* d_digests, uint64_t* counts,
                 dc_replay_stats* stats, const PerGame* per_game = nullptr) {
  const char* name = per_game ? (d_san ? "replay_san_starts" : "replay_outcome_starts")
                              : (d_san ? "replay_san" : "replay_outcome");
  dc_pos s;
  if (start) s = *start;
  else dc_startpos(&s);
  if (s.stm > 1 || start_halfmove > 150) return DC_EINVAL;
  u64 h[dc::kOutcomeRecord] = {};
  if (n_games) {
    const u32 n_blocks = (u32)(((u64)n_games + dc::kOutcomeBlock - 1) / dc::kOutcomeBlock);
    const u32 chunk = (u32)std::min<u64>(chunk_games(c), (u64)n_blocks * dc::kOutcomeBlock);
    HIP_TRY(c->outcome_hist.ensure(dc::outcome_history_words(chunk)));
    HIP_TRY(c->outcome_part.ensure((size_t)dc::kOutcomeRecord * (n_blocks + 1)));
    u64* totals = c->outcome_part.p;
    u64* partial = totals + dc::kOutcomeRecord;
    // the chunks share the history: they run one after another on the stream
    for (u64 first = 0; first < n_games; first += chunk) {
      const u32 count = (u32)std::min<u64>(chunk, n_games - first);
      HIP_TRY(c->timed(name, 0, [&] {
        if (per_game)
          return d_san ? dc::launch_replay_san_starts(c->stream, per_game->starts, per_game->clocks, per_game->finals,
                                                      d_moves, n_games, n_plies, (u32)first, count, c->outcome_hist.p,
                                                      chunk, d_outcomes, d_san, d_bitmap, d_digests, partial)
                       : dc::launch_replay_outcome_starts(c->stream, per_game->starts, per_game->clocks,
                                                          per_game->finals, d_moves, n_games, n_plies, (u32)first,
                                                          count, c->outcome_hist.p, chunk, d_outcomes, d_bitmap,
                                                          d_digests, partial);
        const DevPos& sp = reinterpret_cast<const DevPos&>(s);
        return d_san ? dc::launch_replay_san(c->stream, sp, start_halfmove, d_moves, n_games, n_plies, (u32)first,
                                             count, c->outcome_hist.p, chunk, d_outcomes, d_san, d_bitmap, d_digests,
                                             partial)
                     : dc::launch_replay_outcome(c->stream, sp, start_halfmove, d_moves, n_games, n_plies, (u32)first,
                                                 count, c->outcome_hist.p, chunk, d_outcomes, d_bitmap, d_digests,
                                                 partial);
      }));
    }
    HIP_TRY(dc::launch_outcome_reduce(c->stream, partial, n_blocks, totals));
    HIP_TRY(hipMemcpyAsync(h, totals, sizeof h, hipMemcpyDeviceToHost, c->stream));
  }
  const int r = sync_ctx(c);
  if (r != DC_SUCCESS) return r;
  if (stats) {
    stats->validated = h[0];
    stats->accepted = h[1];
    stats->rejected = h[2];
    stats->digest_sum = h[3];
    stats->digest_xor = h[4];
  }
  if (counts)
    for (u32 k = 0; k < DC_GO_COUNT; ++k) counts[k] = h[5 + k];
  // the unit count: moves consumed (validated plies)
  if (c->profiling && n_games) c->stats[name].units += h[0];
  return DC_SUCCESS;
}

}  // namespace

extern "C" {

static_assert(sizeof(dc_game_outcome) == 8 && DC_GO_COUNT == dc::kOutcomeResults, "dc_game_outcome layout");

int dc_replay_outcome_device(dc_ctx* c, const dc_pos* start, uint32_t start_halfmove, const uint16_t* d_moves,
                             uint32_t n_games, uint32_t n_plies, void* d_outcomes, uint64_t* d_bitmap,
                             uint64_t* d_digests, uint64_t* counts, dc_replay_stats* stats) {
  ENTER_WORK(c);
  if ((n_games && n_plies && !d_moves) || (n_games && !d_outcomes)) return DC_EINVAL;
  return outcome_impl(c, start, start_halfmove, d_moves, n_games, n_plies, static_cast<u64*>(d_outcomes), nullptr,
                      reinterpret_cast<u64*>(d_bitmap), reinterpret_cast<u64*>(d_digests), counts, stats);
}

int dc_replay_outcome(dc_ctx* c, const dc_pos* start, uint32_t start_halfmove, const uint16_t* moves, uint32_t n_games,
                      uint32_t n_plies, void* outcomes, uint64_t* bitmap, uint64_t* digests,
                      uint64_t* counts, dc_replay_stats* stats) {
  ENTER_WORK(c);
  if ((n_games && n_plies && !moves) || (n_games && !outcomes) || start_halfmove > 150) return DC_EINVAL;
  const size_t nm = (size_t)n_games * n_plies;
  const size_t words = (size_t)((n_games + 63) / 64) * n_plies;
  HIP_TRY(c->moves.ensure(std::max<size_t>(nm, 1)));
  HIP_TRY(c->outcomes.ensure(std::max<size_t>(n_games, 1)));
  if (bitmap) HIP_TRY(c->bitmap.ensure(std::max<size_t>(words, 1)));
  if (digests) HIP_TRY(c->digests.ensure(std::max<size_t>(n_games, 1)));
  if (nm) HIP_TRY(hipMemcpyAsync(c->moves.p, moves, nm * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
  const int r = outcome_impl(c, start, start_halfmove, c->moves.p, n_games, n_plies, c->outcomes.p, nullptr,
                             bitmap ? c->bitmap.p : nullptr, digests ? c->digests.p : nullptr, counts, stats);
  if (r != DC_SUCCESS) return r;
  if (n_games)
    HIP_TRY(hipMemcpyAsync(outcomes, c->outcomes.p, (size_t)n_games * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  if (bitmap && words)
    HIP_TRY(hipMemcpyAsync(bitmap, c->bitmap.p, words * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  if (digests && n_games)
    HIP_TRY(hipMemcpyAsync(digests, c->digests.p, (size_t)n_games * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  return sync_ctx(c);
}

// dc_replay_outcome* with the SAN byte of every ply (k_replay_san).
int dc_replay_san_device(dc_ctx* c, const dc_pos* start, uint32_t start_halfmove, const uint16_t* d_moves,
                         uint32_t n_games, uint32_t n_plies, void* d_outcomes, uint8_t* d_san, uint64_t* d_bitmap,
                         uint64_t* d_digests, uint64_t* counts, dc_replay_stats* stats) {
  ENTER_WORK(c);
  if ((n_games && n_plies && (!d_moves || !d_san)) || (n_games && !d_outcomes)) return DC_EINVAL;
  if (!d_san) {  // no plies: nothing is stored, the pointer only selects the kernel
    HIP_TRY(c->san.ensure(1));
    d_san = c->san.p;
  }
  return outcome_impl(c, start, start_halfmove, d_moves, n_games, n_plies, static_cast<u64*>(d_outcomes), d_san,
                      reinterpret_cast<u64*>(d_bitmap), reinterpret_cast<u64*>(d_digests), counts, stats);
}

int dc_replay_san(dc_ctx* c, const dc_pos* start, uint32_t start_halfmove, const uint16_t* moves, uint32_t n_games,
                  uint32_t n_plies, void* outcomes, uint8_t* san, uint64_t* bitmap, uint64_t* digests,
                  uint64_t* counts, dc_replay_stats* stats) {
  ENTER_WORK(c);
  if ((n_games && n_plies && (!moves || !san)) || (n_games && !outcomes) || start_halfmove > 150) return DC_EINVAL;
  const size_t nm = (size_t)n_games * n_plies;
  const size_t words = (size_t)((n_games + 63) / 64) * n_plies;
  HIP_TRY(c->moves.ensure(std::max<size_t>(nm, 1)));
  HIP_TRY(c->san.ensure(std::max<size_t>(nm, 1)));
  HIP_TRY(c->outcomes.ensure(std::max<size_t>(n_games, 1)));
  if (bitmap) HIP_TRY(c->bitmap.ensure(std::max<size_t>(words, 1)));
  if (digests) HIP_TRY(c->digests.ensure(std::max<size_t>(n_games, 1)));
  if (nm) HIP_TRY(hipMemcpyAsync(c->moves.p, moves, nm * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
  const int r = outcome_impl(c, start, start_halfmove, c->moves.p, n_games, n_plies, c->outcomes.p, c->san.p,
                             bitmap ? c->bitmap.p : nullptr, digests ? c->digests.p : nullptr, counts, stats);
  if (r != DC_SUCCESS) return r;
  if (n_games)
    HIP_TRY(hipMemcpyAsync(outcomes, c->outcomes.p, (size_t)n_games * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  if (nm) HIP_TRY(hipMemcpyAsync(san, c->san.p, nm, hipMemcpyDeviceToHost, c->stream));
  if (bitmap && words)
    HIP_TRY(hipMemcpyAsync(bitmap, c->bitmap.p, words * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  if (digests && n_games)
    HIP_TRY(hipMemcpyAsync(digests, c->digests.p, (size_t)n_games * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  return sync_ctx(c);
}

// ---- the per-game-start forms: a start position and a clock per game in, the
// position each game stopped in out.

// The host forms' check of the per-game inputs, before any device work.
static bool starts_valid(const dc_pos* starts, const uint16_t* start_halfmoves, uint32_t n_games) {
  for (uint32_t g = 0; g < n_games; ++g)
    if ((starts && starts[g].stm > 1) || (start_halfmoves && start_halfmoves[g] > 150)) return false;
  return true;
}

// Stages the host forms' starts and clocks through the context's buffers and
// points pg at them (and at the staged finals, if wanted).
static int stage_per_game(dc_ctx* c, const dc_pos* starts, const uint16_t* start_halfmoves, bool want_finals,
                          uint32_t n_games, PerGame* pg) {
  *pg = PerGame{nullptr, nullptr, nullptr};
  if (!n_games) return DC_SUCCESS;
  if (starts) {
    HIP_TRY(c->pos.ensure(n_games));
    HIP_TRY(hipMemcpyAsync(c->pos.p, starts, (size_t)n_games * sizeof(dc_pos), hipMemcpyHostToDevice, c->stream));
    pg->starts = c->pos.p;
  }
  if (start_halfmoves) {
    HIP_TRY(c->start_clocks.ensure(n_games));
    HIP_TRY(hipMemcpyAsync(c->start_clocks.p, start_halfmoves, (size_t)n_games * sizeof(uint16_t),
                           hipMemcpyHostToDevice, c->stream));
    pg->clocks = c->start_clocks.p;
  }
  if (want_finals) {
    HIP_TRY(c->finals.ensure(n_games));
    pg->finals = c->finals.p;
  }
  return DC_SUCCESS;
}

int dc_replay_outcome_starts_device(dc_ctx* c, const dc_pos* d_starts, const uint16_t* d_start_halfmoves,
                                    const uint16_t* d_moves, uint32_t n_games, uint32_t n_plies, void* d_outcomes,
                                    uint64_t* d_bitmap, uint64_t* d_digests, uint64_t* counts, dc_replay_stats* stats,
                                    dc_pos* d_finals) {
  ENTER_WORK(c);
  if ((n_games && n_plies && !d_moves) || (n_games && !d_outcomes)) return DC_EINVAL;
  const PerGame pg{reinterpret_cast<const DevPos*>(d_starts), d_start_halfmoves, reinterpret_cast<DevPos*>(d_finals)};
  return outcome_impl(c, nullptr, 0, d_moves, n_games, n_plies, static_cast<u64*>(d_outcomes), nullptr,
                      reinterpret_cast<u64*>(d_bitmap), reinterpret_cast<u64*>(d_digests), counts, stats, &pg);
}

int dc_replay_san_starts_device(dc_ctx* c, const dc_pos* d_starts, const uint16_t* d_start_halfmoves,
                                const uint16_t* d_moves, uint32_t n_games, uint32_t n_plies, void* d_outcomes,
                                uint8_t* d_san, uint64_t* d_bitmap, uint64_t* d_digests, uint64_t* counts,
                                dc_replay_stats* stats, dc_pos* d_finals) {
  ENTER_WORK(c);
  if ((n_games && n_plies && (!d_moves || !d_san)) || (n_games && !d_outcomes)) return DC_EINVAL;
  if (!d_san) {  // no plies: nothing is stored, the pointer only selects the kernel
    HIP_TRY(c->san.ensure(1));
    d_san = c->san.p;
  }
  const PerGame pg{reinterpret_cast<const DevPos*>(d_starts), d_start_halfmoves, reinterpret_cast<DevPos*>(d_finals)};
  return outcome_impl(c, nullptr, 0, d_moves, n_games, n_plies, static_cast<u64*>(d_outcomes), d_san,
                      reinterpret_cast<u64*>(d_bitmap), reinterpret_cast<u64*>(d_digests), counts, stats, &pg);
}

// Both host forms: san == nullptr is dc_replay_outcome_starts.
static int replay_starts_host(dc_ctx* c, bool with_san, const dc_pos* starts, const uint16_t* start_halfmoves,
                              const uint16_t* moves, uint32_t n_games, uint32_t n_plies, void* outcomes, uint8_t* san,
                              uint64_t* bitmap, uint64_t* digests, uint64_t* counts, dc_replay_stats* stats,
                              dc_pos* finals) {
  if ((n_games && n_plies && (!moves || (with_san && !san))) || (n_games && !outcomes) ||
      !starts_valid(starts, start_halfmoves, n_games))
    return DC_EINVAL;
  const size_t nm = (size_t)n_games * n_plies;
  const size_t words = (size_t)((n_games + 63) / 64) * n_plies;
  HIP_TRY(c->moves.ensure(std::max<size_t>(nm, 1)));
  if (with_san) HIP_TRY(c->san.ensure(std::max<size_t>(nm, 1)));
  HIP_TRY(c->outcomes.ensure(std::max<size_t>(n_games, 1)));
  if (bitmap) HIP_TRY(c->bitmap.ensure(std::max<size_t>(words, 1)));
  if (digests) HIP_TRY(c->digests.ensure(std::max<size_t>(n_games, 1)));
  PerGame pg;
  int r = stage_per_game(c, starts, start_halfmoves, finals != nullptr, n_games, &pg);
  if (r != DC_SUCCESS) return r;
  if (nm) HIP_TRY(hipMemcpyAsync(c->moves.p, moves, nm * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
  r = outcome_impl(c, nullptr, 0, c->moves.p, n_games, n_plies, c->outcomes.p, with_san ? c->san.p : nullptr,
                   bitmap ? c->bitmap.p : nullptr, digests ? c->digests.p : nullptr, counts, stats, &pg);
  if (r != DC_SUCCESS) return r;
  if (n_games)
    HIP_TRY(hipMemcpyAsync(outcomes, c->outcomes.p, (size_t)n_games * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  if (with_san && nm) HIP_TRY(hipMemcpyAsync(san, c->san.p, nm, hipMemcpyDeviceToHost, c->stream));
  if (bitmap && words)
    HIP_TRY(hipMemcpyAsync(bitmap, c->bitmap.p, words * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  if (digests && n_games)
    HIP_TRY(hipMemcpyAsync(digests, c->digests.p, (size_t)n_games * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  if (finals && n_games)
    HIP_TRY(hipMemcpyAsync(finals, c->finals.p, (size_t)n_games * sizeof(dc_pos), hipMemcpyDeviceToHost, c->stream));
  return sync_ctx(c);
}

int dc_replay_outcome_starts(dc_ctx* c, const dc_pos* starts, const uint16_t* start_halfmoves, const uint16_t* moves,
                             uint32_t n_games, uint32_t n_plies, void* outcomes, uint64_t* bitmap, uint64_t* digests,
                             uint64_t* counts, dc_replay_stats* stats, dc_pos* finals) {
  ENTER_WORK(c);
  return replay_starts_host(c, false, starts, start_halfmoves, moves, n_games, n_plies, outcomes, nullptr, bitmap,
                            digests, counts, stats, finals);
}

int dc_replay_san_starts(dc_ctx* c, const dc_pos* starts, const uint16_t* start_halfmoves, const uint16_t* moves,
                         uint32_t n_games, uint32_t n_plies, void* outcomes, uint8_t* san, uint64_t* bitmap,
                         uint64_t* digests, uint64_t* counts, dc_replay_stats* stats, dc_pos* finals) {
  ENTER_WORK(c);
  return replay_starts_host(c, true, starts, start_halfmoves, moves, n_games, n_plies, outcomes, san, bitmap, digests,
                            counts, stats, finals);
}

// The FEN's fifth and sixth fields (half-move clock, full-move number) on the
// host; dc_pos_from_fen reads the first four.  Absent fields give 0 and 1.
int dc_fen_clocks(const char* fen, uint32_t* halfmove, uint32_t* fullmove) {
  if (!fen) return DC_EINVAL;
  const char* s = fen;
  while (*s == ' ') ++s;
  for (int field = 0; field < 4; ++field) {  // placement, side, castling, en passant
    while (*s && *s != ' ') ++s;
    while (*s == ' ') ++s;
  }
  uint32_t v[2] = {0, 1};
  for (int k = 0; k < 2 && *s; ++k) {
    uint64_t x = 0;
    if (*s < '0' || *s > '9') return DC_EINVAL;
    for (; *s >= '0' && *s <= '9'; ++s) {
      x = x * 10 + (uint64_t)(*s - '0');
      if (x > 0xFFFFFFFFull) return DC_EINVAL;
    }
    if (*s && *s != ' ') return DC_EINVAL;
    while (*s == ' ') ++s;
    v[k] = (uint32_t)x;
  }
  if (halfmove) *halfmove = v[0];
  if (fullmove) *fullmove = v[1];
  return DC_SUCCESS;
}

// Test hook (not in the header): the games adjudicated per launch (rounded down
// to whole blocks, at least one), so a test can split a small batch into
// several chunks that share the history buffer.
__attribute__((visibility("default"))) int dc_test_outcome_chunk_games(dc_ctx* c, uint32_t games) {
  if (!c) return DC_EINVAL;
  c->outcome_chunk_games = games;
  return DC_SUCCESS;
}

}  // extern "C"
