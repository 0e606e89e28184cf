// dc_api_resolve.hip -- SAN tokens to move words on the device (dc_san_resolve*).
#include <cstring>

#include "dc_ctx.h"
#include "dc_san_resolve.h"

namespace {

// The kernel, its five counters and the unit count; n_games, and n_plies unless
// per_game: k_starts_san_resolve with d_starts (null: s for all) and d_finals
// (null: not wanted).
int resolve_impl(dc_ctx* c, const dc_pos& s, bool per_game, const DevPos* d_starts, DevPos* d_finals,
                 const uint32_t* d_tokens, uint32_t n_games, uint32_t n_plies, uint16_t* d_moves,
                 uint32_t* d_first_bad, uint64_t* counts) {
  const char* name = per_game ? "san_resolve_starts" : "san_resolve";
  u64 h[dc::kResolveCounts] = {};
  HIP_TRY(c->san_counts.ensure(dc::kResolveCounts));
  HIP_TRY(hipMemsetAsync(c->san_counts.p, 0, sizeof h, c->stream));
  HIP_TRY(c->timed(name, 0, [&] {
    return dc::launch_san_resolve(c->stream, reinterpret_cast<const DevPos&>(s), per_game, d_starts, d_finals,
                                  d_tokens, n_games, n_plies, d_moves, d_first_bad, c->san_counts.p);
  }));
  HIP_TRY(hipMemcpyAsync(h, c->san_counts.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
  const int r = sync_ctx(c);
  if (r != DC_SUCCESS) return r;
  if (counts) std::memcpy(counts, h, sizeof h);
  // the unit count: tokens other than NONE
  if (c->profiling) c->stats[name].units += h[DC_SR_TOKENS];
  return DC_SUCCESS;
}

// The shared start (null: the start position) into s; starts: the per-game
// host form's, null or n of them.
bool starts_valid(const dc_pos* start, const dc_pos* starts, uint32_t n, dc_pos& s) {
  if (start) s = *start;
  else dc_startpos(&s);
  for (uint32_t g = 0; starts && g < n; ++g)
    if (starts[g].stm > 1) return false;
  return s.stm <= 1;
}

// Both device forms; per_game passes no start.  Without plies no ply has a
// flagged word, first_bad = n_plies = 0: the shared form writes that itself, the
// per-game form's kernel still runs, since it also copies the starts to the finals.
int resolve_device(dc_ctx* c, bool per_game, const dc_pos* start, const dc_pos* d_starts, dc_pos* d_finals,
                   const uint32_t* d_tokens, uint32_t n_games, uint32_t n_plies, uint16_t* d_moves,
                   uint32_t* d_first_bad, uint64_t* counts) {
  dc_pos s;
  if (!starts_valid(start, nullptr, 0, s) || (n_games && n_plies && (!d_tokens || !d_moves))) return DC_EINVAL;
  if (counts) std::memset(counts, 0, DC_SR_COUNT * sizeof(uint64_t));
  if (n_games == 0) return DC_SUCCESS;
  if (!per_game && n_plies == 0) {
    if (d_first_bad) HIP_TRY(hipMemsetAsync(d_first_bad, 0, (size_t)n_games * sizeof(uint32_t), c->stream));
    return sync_ctx(c);
  }
  return resolve_impl(c, s, per_game, reinterpret_cast<const DevPos*>(d_starts), reinterpret_cast<DevPos*>(d_finals),
                      d_tokens, n_games, n_plies, d_moves, d_first_bad, counts);
}

// Both host forms; per_game passes no start but its starts and finals (each
// may be null).  No plies: as resolve_device.
int resolve_host(dc_ctx* c, bool per_game, const dc_pos* start, const dc_pos* starts, dc_pos* finals,
                 const uint32_t* tokens, uint32_t n_games, uint32_t n_plies, uint16_t* moves, uint32_t* first_bad,
                 uint64_t* counts) {
  dc_pos s;
  if (!starts_valid(start, starts, n_games, s) || (n_games && n_plies && (!tokens || !moves))) return DC_EINVAL;
  if (counts) std::memset(counts, 0, DC_SR_COUNT * sizeof(uint64_t));
  if (n_games == 0) return DC_SUCCESS;
  if (!per_game && n_plies == 0) {
    if (first_bad) std::memset(first_bad, 0, (size_t)n_games * sizeof(uint32_t));
    return DC_SUCCESS;
  }
  const size_t nm = (size_t)n_games * n_plies;
  HIP_TRY(c->san_tokens.ensure(std::max<size_t>(nm, 1)));
  HIP_TRY(c->moves.ensure(std::max<size_t>(nm, 1)));
  if (first_bad) HIP_TRY(c->san_first_bad.ensure(n_games));
  if (starts) {
    HIP_TRY(c->pos.ensure(n_games));
    HIP_TRY(hipMemcpyAsync(c->pos.p, starts, (size_t)n_games * sizeof(dc_pos), hipMemcpyHostToDevice, c->stream));
  }
  if (finals) HIP_TRY(c->finals.ensure(n_games));
  if (nm) HIP_TRY(hipMemcpyAsync(c->san_tokens.p, tokens, nm * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  const int r = resolve_impl(c, s, per_game, starts ? c->pos.p : nullptr, finals ? c->finals.p : nullptr,
                             c->san_tokens.p, n_games, n_plies, c->moves.p, first_bad ? c->san_first_bad.p : nullptr,
                             counts);
  if (r != DC_SUCCESS) return r;
  if (nm) HIP_TRY(hipMemcpyAsync(moves, c->moves.p, nm * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream));
  if (first_bad)
    HIP_TRY(hipMemcpyAsync(first_bad, c->san_first_bad.p, (size_t)n_games * sizeof(uint32_t), hipMemcpyDeviceToHost,
                           c->stream));
  if (finals)
    HIP_TRY(hipMemcpyAsync(finals, c->finals.p, (size_t)n_games * sizeof(dc_pos), hipMemcpyDeviceToHost, c->stream));
  return sync_ctx(c);
}

}  // namespace

extern "C" {

static_assert(DC_SR_COUNT == dc::kResolveCounts, "dc_san_resolve counters");

int dc_san_resolve_device(dc_ctx* c, const dc_pos* start, const uint32_t* d_tokens, uint32_t n_games,
                          uint32_t n_plies, uint16_t* d_moves, uint32_t* d_first_bad, uint64_t* counts) {
  ENTER_WORK(c);
  return resolve_device(c, false, start, nullptr, nullptr, d_tokens, n_games, n_plies, d_moves, d_first_bad, counts);
}

int dc_san_resolve(dc_ctx* c, const dc_pos* start, const uint32_t* tokens, uint32_t n_games, uint32_t n_plies,
                   uint16_t* moves, uint32_t* first_bad, uint64_t* counts) {
  ENTER_WORK(c);
  return resolve_host(c, false, start, nullptr, nullptr, tokens, n_games, n_plies, moves, first_bad, counts);
}

// ---- the per-game-start forms
int dc_san_resolve_starts_device(dc_ctx* c, const dc_pos* d_starts, const uint32_t* d_tokens, uint32_t n_games,
                                 uint32_t n_plies, uint16_t* d_moves, uint32_t* d_first_bad, uint64_t* counts,
                                 dc_pos* d_finals) {
  ENTER_WORK(c);
  return resolve_device(c, true, nullptr, d_starts, d_finals, d_tokens, n_games, n_plies, d_moves, d_first_bad,
                        counts);
}

int dc_san_resolve_starts(dc_ctx* c, const dc_pos* starts, const uint32_t* tokens, uint32_t n_games, uint32_t n_plies,
                          uint16_t* moves, uint32_t* first_bad, uint64_t* counts, dc_pos* finals) {
  ENTER_WORK(c);
  return resolve_host(c, true, nullptr, starts, finals, tokens, n_games, n_plies, moves, first_bad, counts);
}

}  // extern "C"
