// dc_api_resolve.hip -- SAN tokens to move words on the device (dc_san_resolve*).
#include <cstring>

#include "dc_ctx.h"
#include "dc_san_resolve.h"

namespace {

// The kernel, its five counters and the unit count; n_games && n_plies.
int resolve_impl(dc_ctx* c, const dc_pos& s, const uint32_t* d_tokens, uint32_t n_games, uint32_t n_plies,
                 uint16_t* d_moves, uint32_t* d_first_bad, uint64_t* counts) {
  u64 h[dc::kResolveCounts] = {};
  HIP_TRY(c->san_counts.ensure(dc::kResolveCounts));
  HIP_TRY(hipMemsetAsync(c->san_counts.p, 0, sizeof h, c->stream));
  HIP_TRY(c->timed("san_resolve", 0, [&] {
    return dc::launch_san_resolve(c->stream, reinterpret_cast<const DevPos&>(s), d_tokens, n_games, n_plies, d_moves,
                                  d_first_bad, c->san_counts.p);
  }));
  HIP_TRY(hipMemcpyAsync(h, c->san_counts.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
  const int r = sync_ctx(c);
  if (r != DC_SUCCESS) return r;
  if (counts) std::memcpy(counts, h, sizeof h);
  // the unit count: tokens other than NONE
  if (c->profiling) c->stats["san_resolve"].units += h[DC_SR_TOKENS];
  return DC_SUCCESS;
}

bool start_of(const dc_pos* start, dc_pos& s) {
  if (start) s = *start;
  else dc_startpos(&s);
  return s.stm <= 1;
}

}  // namespace

extern "C" {

static_assert(DC_SR_COUNT == dc::kResolveCounts, "dc_san_resolve counters");

int dc_san_resolve_device(dc_ctx* c, const dc_pos* start, const uint32_t* d_tokens, uint32_t n_games,
                          uint32_t n_plies, uint16_t* d_moves, uint32_t* d_first_bad, uint64_t* counts) {
  ENTER_WORK(c);
  dc_pos s;
  if (!start_of(start, s) || (n_games && n_plies && (!d_tokens || !d_moves))) return DC_EINVAL;
  if (counts) std::memset(counts, 0, DC_SR_COUNT * sizeof(uint64_t));
  if (n_games == 0) return DC_SUCCESS;
  if (n_plies == 0) {  // no ply has a flagged word: first_bad = n_plies = 0
    if (d_first_bad) HIP_TRY(hipMemsetAsync(d_first_bad, 0, (size_t)n_games * sizeof(uint32_t), c->stream));
    return sync_ctx(c);
  }
  return resolve_impl(c, s, d_tokens, n_games, n_plies, d_moves, d_first_bad, counts);
}

int dc_san_resolve(dc_ctx* c, const dc_pos* start, const uint32_t* tokens, uint32_t n_games, uint32_t n_plies,
                   uint16_t* moves, uint32_t* first_bad, uint64_t* counts) {
  ENTER_WORK(c);
  dc_pos s;
  if (!start_of(start, s) || (n_games && n_plies && (!tokens || !moves))) return DC_EINVAL;
  if (counts) std::memset(counts, 0, DC_SR_COUNT * sizeof(uint64_t));
  if (n_games == 0) return DC_SUCCESS;
  if (n_plies == 0) {
    if (first_bad) std::memset(first_bad, 0, (size_t)n_games * sizeof(uint32_t));
    return DC_SUCCESS;
  }
  const size_t nm = (size_t)n_games * n_plies;
  HIP_TRY(c->san_tokens.ensure(nm));
  HIP_TRY(c->moves.ensure(nm));
  if (first_bad) HIP_TRY(c->san_first_bad.ensure(n_games));
  HIP_TRY(hipMemcpyAsync(c->san_tokens.p, tokens, nm * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  const int r = resolve_impl(c, s, c->san_tokens.p, n_games, n_plies, c->moves.p,
                             first_bad ? c->san_first_bad.p : nullptr, counts);
  if (r != DC_SUCCESS) return r;
  HIP_TRY(hipMemcpyAsync(moves, c->moves.p, nm * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream));
  if (first_bad)
    HIP_TRY(hipMemcpyAsync(first_bad, c->san_first_bad.p, (size_t)n_games * sizeof(uint32_t), hipMemcpyDeviceToHost,
                           c->stream));
  return sync_ctx(c);
}

}  // extern "C"
