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

using PerGame = dc::OutcomePerGame;  // the *_starts calls' arrays in device memory (each may be null)
// The same three in host memory, as the host forms get them.
struct HostPerGame {
  const dc_pos* starts;
  const uint16_t* clocks;
  dc_pos* finals;
};

// The check of the shared start and clock and of a host form's per-game ones,
// before any device work (a device form's arrays cannot be read here: the
// kernel reads stm & 1 and clamps the clock).
bool starts_valid(const dc_pos* start, uint32_t start_halfmove, const HostPerGame* host, uint32_t n_games) {
  if ((start && start->stm > 1) || start_halfmove > 150) return false;
  for (uint32_t g = 0; host && g < n_games; ++g)
    if ((host->starts && host->starts[g].stm > 1) || (host->clocks && host->clocks[g] > 150)) return false;
  return true;
}

// One adjudicated batch in device memory; the arguments are valid.
// d_san == nullptr: k_replay_outcome; else k_replay_san, which also fills d_san.
// per_game != nullptr: the *_starts kernels instead, with the start position
// where it has no starts and clock 0 where it has no clocks.
int outcome_impl(dc_ctx* c, const dc_pos* start, uint32_t start_halfmove, const uint16_t* d_moves, uint32_t n_games,
                 uint32_t n_plies, u64* d_outcomes, uint8_t* d_san, u64* d_bitmap, u64* d_digests, uint64_t* counts,
                 dc_replay_stats* stats, const PerGame* per_game) {
  const char* name = per_game ? (d_san ? "replay_san_starts" : "replay_outcome_starts")
                              : (d_san ? "replay_san" : "replay_outcome");
  const auto launch = d_san ? dc::launch_replay_san : dc::launch_replay_outcome;
  dc_pos s;
  if (start) s = *start;
  else dc_startpos(&s);
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
      const dc::OutcomeBatch a{d_moves, n_games,    n_plies, (u32)first, count,     c->outcome_hist.p,
                               chunk,   d_outcomes, d_san,   d_bitmap,   d_digests, partial};
      HIP_TRY(c->timed(name, 0, [&] {
        return launch(c->stream, reinterpret_cast<const DevPos&>(s), start_halfmove, per_game, a);
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

// The four *_device entry points.  with_san: the dc_replay_san* ones.
// per_game: the *_starts ones, which pass no start and no clock.
int replay_device(dc_ctx* c, bool with_san, const dc_pos* start, uint32_t start_halfmove, const PerGame* per_game,
                  const uint16_t* d_moves, uint32_t n_games, uint32_t n_plies, void* d_outcomes, uint8_t* d_san,
                  uint64_t* d_bitmap, uint64_t* d_digests, uint64_t* counts, dc_replay_stats* stats) {
  if ((n_games && n_plies && (!d_moves || (with_san && !d_san))) || (n_games && !d_outcomes) ||
      !starts_valid(start, start_halfmove, nullptr, 0))
    return DC_EINVAL;
  if (with_san && !d_san) {  // no plies: nothing is stored, the pointer only selects the kernel
    HIP_TRY(c->san.ensure(1));
    d_san = c->san.p;
  }
  return outcome_impl(c, start, start_halfmove, d_moves, n_games, n_plies, static_cast<u64*>(d_outcomes),
                      with_san ? d_san : nullptr, reinterpret_cast<u64*>(d_bitmap), reinterpret_cast<u64*>(d_digests),
                      counts, stats, per_game);
}

// The four host entry points: the inputs go through the context's buffers to
// outcome_impl, the results come back.  with_san: the dc_replay_san* ones.
// host: the *_starts ones, which pass no start and no clock.
int replay_host(dc_ctx* c, bool with_san, const dc_pos* start, uint32_t start_halfmove, const HostPerGame* host,
                const uint16_t* moves, uint32_t n_games, uint32_t n_plies, void* outcomes, uint8_t* san,
                uint64_t* bitmap, uint64_t* digests, uint64_t* counts, dc_replay_stats* stats) {
  if ((n_games && n_plies && (!moves || (with_san && !san))) || (n_games && !outcomes) ||
      !starts_valid(start, start_halfmove, host, n_games))
    return DC_EINVAL;
  const size_t nm = (size_t)n_games * n_plies;
  const size_t words = (size_t)((n_games + 63) / 64) * n_plies;
  HIP_TRY(c->moves.ensure(std::max<size_t>(nm, 1)));
  if (with_san) HIP_TRY(c->san.ensure(std::max<size_t>(nm, 1)));
  HIP_TRY(c->outcomes.ensure(std::max<size_t>(n_games, 1)));
  if (bitmap) HIP_TRY(c->bitmap.ensure(std::max<size_t>(words, 1)));
  if (digests) HIP_TRY(c->digests.ensure(std::max<size_t>(n_games, 1)));
  PerGame pg{nullptr, nullptr, nullptr};
  if (host && n_games) {
    if (host->starts) {
      HIP_TRY(c->pos.ensure(n_games));
      HIP_TRY(hipMemcpyAsync(c->pos.p, host->starts, (size_t)n_games * sizeof(dc_pos), hipMemcpyHostToDevice,
                             c->stream));
      pg.starts = c->pos.p;
    }
    if (host->clocks) {
      HIP_TRY(c->start_clocks.ensure(n_games));
      HIP_TRY(hipMemcpyAsync(c->start_clocks.p, host->clocks, (size_t)n_games * sizeof(uint16_t),
                             hipMemcpyHostToDevice, c->stream));
      pg.clocks = c->start_clocks.p;
    }
    if (host->finals) {
      HIP_TRY(c->finals.ensure(n_games));
      pg.finals = c->finals.p;
    }
  }
  if (nm) HIP_TRY(hipMemcpyAsync(c->moves.p, moves, nm * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
  const int r = outcome_impl(c, start, start_halfmove, c->moves.p, n_games, n_plies, c->outcomes.p,
                             with_san ? c->san.p : nullptr, bitmap ? c->bitmap.p : nullptr,
                             digests ? c->digests.p : nullptr, counts, stats, host ? &pg : nullptr);
  if (r != DC_SUCCESS) return r;
  if (n_games)
    HIP_TRY(hipMemcpyAsync(outcomes, c->outcomes.p, (size_t)n_games * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  if (with_san && nm) HIP_TRY(hipMemcpyAsync(san, c->san.p, nm, hipMemcpyDeviceToHost, c->stream));
  if (bitmap && words)
    HIP_TRY(hipMemcpyAsync(bitmap, c->bitmap.p, words * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  if (digests && n_games)
    HIP_TRY(hipMemcpyAsync(digests, c->digests.p, (size_t)n_games * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  if (pg.finals)
    HIP_TRY(hipMemcpyAsync(host->finals, c->finals.p, (size_t)n_games * sizeof(dc_pos), hipMemcpyDeviceToHost,
                           c->stream));
  return sync_ctx(c);
}

}  // namespace

extern "C" {

static_assert(sizeof(dc_game_outcome) == 8 && DC_GO_COUNT == dc::kOutcomeResults, "dc_game_outcome layout");

int dc_replay_outcome_device(dc_ctx* c, const dc_pos* start, uint32_t start_halfmove, const uint16_t* d_moves,
                             uint32_t n_games, uint32_t n_plies, void* d_outcomes, uint64_t* d_bitmap,
                             uint64_t* d_digests, uint64_t* counts, dc_replay_stats* stats) {
  ENTER_WORK(c);
  return replay_device(c, false, start, start_halfmove, nullptr, d_moves, n_games, n_plies, d_outcomes, nullptr,
                       d_bitmap, d_digests, counts, stats);
}

int dc_replay_outcome(dc_ctx* c, const dc_pos* start, uint32_t start_halfmove, const uint16_t* moves, uint32_t n_games,
                      uint32_t n_plies, void* outcomes, uint64_t* bitmap, uint64_t* digests,
                      uint64_t* counts, dc_replay_stats* stats) {
  ENTER_WORK(c);
  return replay_host(c, false, start, start_halfmove, nullptr, moves, n_games, n_plies, outcomes, nullptr, bitmap,
                     digests, counts, stats);
}

// dc_replay_outcome* with the SAN byte of every ply (k_replay_san).
int dc_replay_san_device(dc_ctx* c, const dc_pos* start, uint32_t start_halfmove, const uint16_t* d_moves,
                         uint32_t n_games, uint32_t n_plies, void* d_outcomes, uint8_t* d_san, uint64_t* d_bitmap,
                         uint64_t* d_digests, uint64_t* counts, dc_replay_stats* stats) {
  ENTER_WORK(c);
  return replay_device(c, true, start, start_halfmove, nullptr, d_moves, n_games, n_plies, d_outcomes, d_san, d_bitmap,
                       d_digests, counts, stats);
}

int dc_replay_san(dc_ctx* c, const dc_pos* start, uint32_t start_halfmove, const uint16_t* moves, uint32_t n_games,
                  uint32_t n_plies, void* outcomes, uint8_t* san, uint64_t* bitmap, uint64_t* digests,
                  uint64_t* counts, dc_replay_stats* stats) {
  ENTER_WORK(c);
  return replay_host(c, true, start, start_halfmove, nullptr, moves, n_games, n_plies, outcomes, san, bitmap, digests,
                     counts, stats);
}

// ---- the per-game-start forms: a start position and a clock per game in, the
// position each game stopped in out.

int dc_replay_outcome_starts_device(dc_ctx* c, const dc_pos* d_starts, const uint16_t* d_start_halfmoves,
                                    const uint16_t* d_moves, uint32_t n_games, uint32_t n_plies, void* d_outcomes,
                                    uint64_t* d_bitmap, uint64_t* d_digests, uint64_t* counts, dc_replay_stats* stats,
                                    dc_pos* d_finals) {
  ENTER_WORK(c);
  const PerGame pg{reinterpret_cast<const DevPos*>(d_starts), d_start_halfmoves, reinterpret_cast<DevPos*>(d_finals)};
  return replay_device(c, false, nullptr, 0, &pg, d_moves, n_games, n_plies, d_outcomes, nullptr, d_bitmap, d_digests,
                       counts, stats);
}

int dc_replay_san_starts_device(dc_ctx* c, const dc_pos* d_starts, const uint16_t* d_start_halfmoves,
                                const uint16_t* d_moves, uint32_t n_games, uint32_t n_plies, void* d_outcomes,
                                uint8_t* d_san, uint64_t* d_bitmap, uint64_t* d_digests, uint64_t* counts,
                                dc_replay_stats* stats, dc_pos* d_finals) {
  ENTER_WORK(c);
  const PerGame pg{reinterpret_cast<const DevPos*>(d_starts), d_start_halfmoves, reinterpret_cast<DevPos*>(d_finals)};
  return replay_device(c, true, nullptr, 0, &pg, d_moves, n_games, n_plies, d_outcomes, d_san, d_bitmap, d_digests,
                       counts, stats);
}

int dc_replay_outcome_starts(dc_ctx* c, const dc_pos* starts, const uint16_t* start_halfmoves, const uint16_t* moves,
                             uint32_t n_games, uint32_t n_plies, void* outcomes, uint64_t* bitmap, uint64_t* digests,
                             uint64_t* counts, dc_replay_stats* stats, dc_pos* finals) {
  ENTER_WORK(c);
  const HostPerGame host{starts, start_halfmoves, finals};
  return replay_host(c, false, nullptr, 0, &host, moves, n_games, n_plies, outcomes, nullptr, bitmap, digests, counts,
                     stats);
}

int dc_replay_san_starts(dc_ctx* c, const dc_pos* starts, const uint16_t* start_halfmoves, const uint16_t* moves,
                         uint32_t n_games, uint32_t n_plies, void* outcomes, uint8_t* san, uint64_t* bitmap,
                         uint64_t* digests, uint64_t* counts, dc_replay_stats* stats, dc_pos* finals) {
  ENTER_WORK(c);
  const HostPerGame host{starts, start_halfmoves, finals};
  return replay_host(c, true, nullptr, 0, &host, moves, n_games, n_plies, outcomes, san, bitmap, digests, counts,
                     stats);
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
