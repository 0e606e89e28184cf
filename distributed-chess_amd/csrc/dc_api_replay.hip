// dc_api_replay.hip -- replay, the state hash (with dc_history_append and
// dc_keccak256, which share its host helpers) and game generation.
#include <cstring>

#include "dc_ctx.h"
#include "dc_fide.h"
#include "dc_hash.h"
#include "dc_keccak.h"

extern "C" {

// ================================================================== replay
static int replay_impl(dc_ctx* c, uint32_t rules, const dc_pos* start, const uint16_t* d_moves, uint32_t n_games,
                       uint32_t n_plies, u64* d_bitmap, u64* d_digests, dc_replay_stats* stats,
                       uint8_t* d_info = nullptr) {
  dc_pos s;
  if (start) s = *start;
  else dc_startpos(&s);
  if (s.stm > 1) return DC_EINVAL;
  // per-ply info: REF only (FIDE notation would need promotion/castling,
  // which the reference's update_history never sees); one buffer descriptor
  if (d_info && (rules != DC_RULES_REF || (u64)n_games * n_plies * 2 > 0xFFFFFFFFull)) return DC_EUNSUPPORTED;
  // stats5 = [5 totals | partials]; the reduction kernel writes all five totals
  HIP_TRY(c->stats5.ensure(5 + 5 * (size_t)dc::replay_partials(std::max<u32>(n_games, 1))));
  if (!c->replay_host) HIP_TRY(c->replay_host.alloc(hipHostMallocDefault, 5 * sizeof(u64)));
  u64* partial = c->stats5.p + 5;
  const Board b{s.bb[0], s.bb[1], s.bb[2], s.bb[3]};
  bool host_written = false;
  HIP_TRY(c->timed("replay", (u64)n_games * n_plies, [&] {
    return rules == DC_RULES_REF
               ? dc::launch_replay_ref(c->stream, b, s.stm, d_moves, n_games, n_plies, d_bitmap, d_digests, c->stats5.p,
                                       partial, c->replay_host, &host_written, d_info)
               : dc::launch_replay_fide(c->stream, reinterpret_cast<const DevPos&>(s), d_moves, n_games, n_plies,
                                        d_bitmap, d_digests, c->stats5.p, partial);
  }));
  u64 h[5] = {0, 0, 0, 0, 0};
  if (!host_written && n_games)
    HIP_TRY(hipMemcpyAsync(h, c->stats5.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
  int r = sync_ctx(c);
  if (r != DC_SUCCESS) return r;
  if (host_written) std::memcpy(h, c->replay_host, sizeof h);
  if (stats) {
    stats->validated = h[0];
    stats->accepted = h[1];
    stats->rejected = h[2];
    stats->digest_sum = h[3];
    stats->digest_xor = h[4];
  }
  // patch the unit count to validated moves (non-sentinel plies)
  if (c->profiling) {
    auto& ks = c->stats["replay"];
    ks.units = ks.units - (u64)n_games * n_plies + h[0];
  }
  return DC_SUCCESS;
}

int dc_replay_device(dc_ctx* c, uint32_t rules, const dc_pos* start, const uint16_t* d_moves, uint32_t n_games,
                     uint32_t n_plies, uint64_t* d_bitmap, uint64_t* d_digests, dc_replay_stats* stats) {
  ENTER_WORK(c);
  if (rules > DC_RULES_FIDE || (n_games && n_plies && !d_moves)) return DC_EINVAL;
  return replay_impl(c, rules, start, d_moves, n_games, n_plies, reinterpret_cast<u64*>(d_bitmap),
                     reinterpret_cast<u64*>(d_digests), stats);
}

int dc_replay(dc_ctx* c, uint32_t rules, const dc_pos* start, const uint16_t* moves, uint32_t n_games,
              uint32_t n_plies, uint64_t* bitmap, uint64_t* digests, dc_replay_stats* stats) {
  ENTER_WORK(c);
  if (rules > DC_RULES_FIDE || (n_games && n_plies && !moves)) return DC_EINVAL;
  const size_t nm = (size_t)n_games * n_plies;
  const size_t words = (size_t)((n_games + 63) / 64) * n_plies;
  HIP_TRY(c->moves.ensure(std::max<size_t>(nm, 1)));
  if (bitmap) HIP_TRY(c->bitmap.ensure(std::max<size_t>(words, 1)));
  if (digests) HIP_TRY(c->digests.ensure(std::max<size_t>(n_games, 1)));
  if (nm) HIP_TRY(hipMemcpyAsync(c->moves.p, moves, nm * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
  int r = replay_impl(c, rules, start, c->moves.p, n_games, n_plies, bitmap ? c->bitmap.p : nullptr,
                      digests ? c->digests.p : nullptr, stats);
  if (r != DC_SUCCESS) return r;
  if (bitmap && words)
    HIP_TRY(hipMemcpyAsync(bitmap, c->bitmap.p, words * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  if (digests && n_games)
    HIP_TRY(hipMemcpyAsync(digests, c->digests.p, (size_t)n_games * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  return sync_ctx(c);
}

int dc_replay_info_device(dc_ctx* c, uint32_t rules, const dc_pos* start, const uint16_t* d_moves, uint32_t n_games,
                          uint32_t n_plies, uint64_t* d_bitmap, uint64_t* d_digests, uint8_t* d_info,
                          dc_replay_stats* stats) {
  ENTER_WORK(c);
  if (rules > DC_RULES_FIDE || (n_games && n_plies && (!d_moves || !d_info))) return DC_EINVAL;
  return replay_impl(c, rules, start, d_moves, n_games, n_plies, reinterpret_cast<u64*>(d_bitmap),
                     reinterpret_cast<u64*>(d_digests), stats, d_info);
}

int dc_replay_info(dc_ctx* c, uint32_t rules, const dc_pos* start, const uint16_t* moves, uint32_t n_games,
                   uint32_t n_plies, uint64_t* bitmap, uint64_t* digests, uint8_t* info, dc_replay_stats* stats) {
  ENTER_WORK(c);
  if (rules > DC_RULES_FIDE || (n_games && n_plies && (!moves || !info))) return DC_EINVAL;
  if (rules != DC_RULES_REF) return DC_EUNSUPPORTED;
  const size_t nm = (size_t)n_games * n_plies;
  // replay_impl's limit (n_games * n_plies * 2 < 4 GiB), checked before any
  // buffer is sized or any byte is copied
  if (nm * 2 >= (1ull << 32)) return DC_EUNSUPPORTED;
  const size_t words = (size_t)((n_games + 63) / 64) * n_plies;
  HIP_TRY(c->moves.ensure(std::max<size_t>(nm, 1)));
  HIP_TRY(c->replay_info.ensure(std::max<size_t>(nm, 1)));
  if (bitmap) HIP_TRY(c->bitmap.ensure(std::max<size_t>(words, 1)));
  if (digests) HIP_TRY(c->digests.ensure(std::max<size_t>(n_games, 1)));
  if (nm) HIP_TRY(hipMemcpyAsync(c->moves.p, moves, nm * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
  int r = replay_impl(c, rules, start, c->moves.p, n_games, n_plies, bitmap ? c->bitmap.p : nullptr,
                      digests ? c->digests.p : nullptr, stats, c->replay_info.p);
  if (r != DC_SUCCESS) return r;
  if (nm) HIP_TRY(hipMemcpyAsync(info, c->replay_info.p, nm, hipMemcpyDeviceToHost, c->stream));
  if (bitmap && words)
    HIP_TRY(hipMemcpyAsync(bitmap, c->bitmap.p, words * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  if (digests && n_games)
    HIP_TRY(hipMemcpyAsync(digests, c->digests.p, (size_t)n_games * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  return sync_ctx(c);
}

// ------------------------------------------------------------ state hashes
}  // extern "C"

namespace {

// serde_json's string escaping (serde_json 1.0 ser.rs ESCAPE table): '"' and
// '\\', \b \t \n \f \r, other bytes < 0x20 as \u00xx (lowercase hex); every
// other byte, UTF-8 included, verbatim.
void json_escape(const char* s, size_t n, std::string& out) {
  static const char hex[] = "0123456789abcdef";
  size_t clean = 0;  // fast path: a run of bytes that need no escape is appended whole
  while (clean < n) {
    const unsigned char ch = (unsigned char)s[clean];
    if (ch < 0x20 || ch == '"' || ch == '\\') break;
    ++clean;
  }
  out.append(s, clean);
  for (size_t i = clean; i < n; ++i) {
    const unsigned char ch = (unsigned char)s[i];
    switch (ch) {
      case '"': out += "\\\""; break;
      case '\\': out += "\\\\"; break;
      case '\b': out += "\\b"; break;
      case '\t': out += "\\t"; break;
      case '\n': out += "\\n"; break;
      case '\f': out += "\\f"; break;
      case '\r': out += "\\r"; break;
      default:
        if (ch < 0x20) {
          out += "\\u00";
          out += hex[ch >> 4];
          out += hex[ch & 15];
        } else {
          out += (char)ch;
        }
    }
  }
}

// Rust's str::split_whitespace().count() (char::is_whitespace = Unicode White_Space).
u32 count_ws_tokens(const char* s, size_t n) {
  auto is_ws = [](u32 c) {
    return (c >= 9 && c <= 13) || c == 32 || c == 0x85 || c == 0xA0 || c == 0x1680 || (c >= 0x2000 && c <= 0x200A) ||
           c == 0x2028 || c == 0x2029 || c == 0x202F || c == 0x205F || c == 0x3000;
  };
  u32 count = 0;
  bool in_tok = false;
  for (size_t i = 0; i < n;) {
    const unsigned char b0 = (unsigned char)s[i];
    u32 c = b0, len = 1;
    if (b0 >= 0xF0) { c = b0 & 7; len = 4; }
    else if (b0 >= 0xE0) { c = b0 & 15; len = 3; }
    else if (b0 >= 0xC0) { c = b0 & 31; len = 2; }
    for (u32 k = 1; k < len && i + k < n; ++k) c = (c << 6) | ((unsigned char)s[i + k] & 63);
    i += len;
    const bool ws = is_ws(c);
    if (!ws && !in_tok) ++count;
    in_tok = !ws;
  }
  return count;
}

// Enqueues the names check of stage_hash_text: k_names_plain's flag (0: no
// byte of any name needs escaping and the offsets are ordered) is read back
// into pinned memory, then plain_ev is recorded.  state_hash_impl enqueues it
// ahead of the replay pre-pass, so the host's wait for the flag ends while the
// GPU still runs the pass and the hash kernel is enqueued behind the pass
// (round 6: a stream-wide wait after the pass left the GPU idle between the
// two kernels).
int begin_names_check(dc_ctx* c, const char* d_names, const uint32_t* d_names_off, uint32_t n_games) {
  const u64 n_str = 2ull * n_games;
  if (n_str + 1 > 0x7FFFFFFFull) return DC_EUNSUPPORTED;  // hipcub's item count is an int
  if (!c->plain_host) HIP_TRY(c->plain_host.alloc());
  if (!c->plain_ev) HIP_TRY(hipEventCreateWithFlags(&c->plain_ev.h, hipEventDisableTiming));
  HIP_TRY(c->esc_lens.ensure(n_str + 1));
  HIP_TRY(dc::launch_names_plain(c->stream, d_names, d_names_off, (u32)n_str, c->esc_lens.p));
  HIP_TRY(hipMemcpyAsync(c->plain_host, c->esc_lens.p, sizeof(u32), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipEventRecord(c->plain_ev, c->stream));
  return DC_SUCCESS;
}

// Stages the hash kernel's text on the device: hash_text = the start history
// escaped on the host (one string per batch) followed by the player names
// escaped on the device from the raw UTF-8 in d_names (serde_json's table,
// k_escape_len / k_escape_write); hash_off = the names' escaped offsets.  One
// small readback sizes hash_text from the exact escaped total.  Runs after
// begin_names_check.
int stage_hash_text(dc_ctx* c, const char* history, const char* d_names, const uint32_t* d_names_off, uint32_t n_games,
                    u32* hist_len, u32* hist_tokens, const char** names_out, const u32** off_out) {
  const size_t hn = history ? std::strlen(history) : 0;
  c->hist_text.clear();
  json_escape(history ? history : "", hn, c->hist_text);
  if (c->hist_text.size() > 0xFFFFFFFFull) return DC_EUNSUPPORTED;
  *hist_len = (u32)c->hist_text.size();
  *hist_tokens = count_ws_tokens(history ? history : "", hn);
  const u64 n_str = 2ull * n_games;
  // Fast path (round 6): names with no byte to escape and ordered offsets are
  // their own serde_json escapes; the hash kernel then reads them in place and
  // the escaping kernels, scan and copy (~80 us per 1M games) are skipped.
  HIP_TRY(hipEventSynchronize(c->plain_ev));
  const u32 escapes = *c->plain_host;
  if (!escapes) {
    HIP_TRY(c->hash_text.ensure(std::max<size_t>(*hist_len, 1)));
    if (*hist_len)
      HIP_TRY(hipMemcpyAsync(c->hash_text.p, c->hist_text.data(), *hist_len, hipMemcpyHostToDevice, c->stream));
    *names_out = d_names;
    *off_out = d_names_off;
    return DC_SUCCESS;
  }
  const size_t tb = dc::escape_scan_tmp_bytes((u32)n_str);
  HIP_TRY(c->esc64.ensure(n_str + 1));
  HIP_TRY(c->scan_tmp.ensure(std::max<size_t>(tb, 1)));
  HIP_TRY(c->hash_off.ensure(n_str + 1));
  HIP_TRY(dc::launch_escape_len_scan(c->stream, d_names, d_names_off, (u32)n_str, *hist_len, c->esc_lens.p,
                                     c->scan_tmp.p, tb, c->esc64.p));
  u64 total = 0;
  HIP_TRY(hipMemcpyAsync(&total, c->esc64.p + n_str, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (total > 0xFFFFFFFFull) return DC_EUNSUPPORTED;  // the hash kernel's offsets are u32
  HIP_TRY(c->hash_text.ensure(std::max<size_t>(total, 1)));
  if (*hist_len)
    HIP_TRY(hipMemcpyAsync(c->hash_text.p, c->hist_text.data(), *hist_len, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(dc::launch_escape_write(c->stream, d_names, d_names_off, (u32)n_str, c->esc64.p, c->hash_off.p,
                                  c->hash_text.p));
  *names_out = c->hash_text.p;
  *off_out = c->hash_off.p;
  return DC_SUCCESS;
}

int state_hash_impl(dc_ctx* c, const dc_pos* start, const char* history, const char* d_names,
                    const uint32_t* d_names_off, const uint16_t* d_moves, uint32_t n_games, uint32_t n_plies,
                    uint8_t* d_hashes) {
  if (!d_names_off || (n_games && n_plies && !d_moves) || (n_games && !d_hashes)) return DC_EINVAL;
  dc_pos s0;
  if (start) s0 = *start;
  else dc_startpos(&s0);
  if (s0.stm > 1) return DC_EINVAL;
  // pieces of unknown kind keep a proto kind string this engine does not know
  if (s0.bb[3] & ~(s0.bb[1] | s0.bb[2])) return DC_EUNSUPPORTED;
  if (n_games == 0) return DC_SUCCESS;
  const Board b{s0.bb[0], s0.bb[1], s0.bb[2], s0.bb[3]};
  // The replay kernel first (round 5): its per-ply info byte (dc_replay_info's
  // form) gives the hash kernel each ply's verdict, mover kind and capture, so
  // the hash kernel validates nothing.  Batches past the replay kernel's one
  // buffer descriptor keep the hash kernel's own validation pass.
  const uint8_t* d_info = nullptr;
  {
    const int e = begin_names_check(c, d_names, d_names_off, n_games);
    if (e != DC_SUCCESS) return e;
  }
  // The pre-pass is an optimisation: when its buffers (up to ~2 GiB near the
  // move bound) cannot be had, or exceed the context's pre-pass budget (a test
  // hook), the hash kernel validates on its own instead of the call failing.
  // (round 6: the pass also leaves every game's final board, 32 B a game,
  // so the hash kernel makes no move)
  const u64 pre_bytes = (u64)n_games * n_plies + 8 * (5 + 5 * (u64)dc::replay_partials(n_games)) +
                        sizeof(Board) * (u64)n_games;
  bool pre = n_plies > 0 && (u64)n_games * n_plies * 2 <= 0xFFFFFFFFull && pre_bytes <= c->hash_prepass_max;
  if (pre && (c->replay_info.ensure((size_t)n_games * n_plies) != hipSuccess ||
              c->hash_boards.ensure(n_games) != hipSuccess ||
              c->stats5.ensure(5 + 5 * (size_t)dc::replay_partials(n_games)) != hipSuccess)) {
    (void)hipGetLastError();
    pre = false;
  }
  const Board* d_boards = nullptr;
  if (pre) {
    bool host_written = false;
    HIP_TRY(c->timed("state_hash_replay", (u64)n_games * n_plies, [&] {
      return dc::launch_replay_ref(c->stream, b, s0.stm, d_moves, n_games, n_plies, nullptr, nullptr, c->stats5.p,
                                   c->stats5.p + 5, nullptr, &host_written, c->replay_info.p, c->hash_boards.p);
    }));
    d_info = c->replay_info.p;
    d_boards = c->hash_boards.p;
  }
  // the names staged after the pass is enqueued: the staging waits only for the
  // names check enqueued ahead of the pass (begin_names_check), so the hash
  // kernel is enqueued while the GPU runs the pass (round 6)
  u32 hist_len = 0, hist_tokens = 0;
  const char* names = nullptr;
  const u32* names_off = nullptr;
  int e = stage_hash_text(c, history, d_names, d_names_off, n_games, &hist_len, &hist_tokens, &names, &names_off);
  if (e != DC_SUCCESS) return e;
  const char* text = c->hash_text.p;
  HIP_TRY(c->timed("state_hash", n_games, [&] {
    return dc::launch_state_hash_ref(c->stream, b, s0.stm, d_moves, n_games, n_plies, text, hist_len, hist_tokens,
                                     names, names_off, d_info, d_hashes, d_boards, c->hash_bcd_max);
  }));
  return sync_ctx(c);
}

}  // namespace

extern "C" {

// update_history (chess.rs:127-184) for one game's accepted plies, on the
// host: the reference's notation (convert_move_to_notation, :134-154) with its
// numbering quirk -- the move number is 1 + the number of whitespace-separated
// tokens already in the history (:169-183), so it runs 1, 3, 5, ... from "".
int dc_history_append(const char* history, const uint16_t* moves, const uint8_t* info, uint32_t n_plies,
                      size_t stride, char* out, size_t out_cap, size_t* out_len) {
  if ((n_plies && (!moves || !info)) || !out_len || (out_cap && !out)) return DC_EINVAL;
  if (stride == 0) stride = 1;
  std::string h = history ? history : "";
  size_t tokens = count_ws_tokens(h.c_str(), h.size());  // split_whitespace().count()
  static const char* kKind[7] = {"", "N", "B", "R", "Q", "K", ""};
  for (uint32_t p = 0; p < n_plies; ++p) {
    const uint8_t code = info[(size_t)p * stride];
    const uint16_t m = moves[(size_t)p * stride];
    if (code == 0xFF) continue;  // rejected or padded: not applied, no history entry
    if ((code & 7) > 5) return DC_EUNSUPPORTED;  // an OTHER piece never moves (chess.rs:210)
    const int f = m & 63, t = (m >> 6) & 63;
    std::string san = kKind[code & 7];
    if (code & 8) {
      if ((code & 7) == 0) san += (char)('a' + (f & 7));
      san += 'x';
    }
    san += (char)('a' + (t & 7));
    san += std::to_string((t >> 3) + 1);
    h += (tokens == 0 ? "" : " ") + std::to_string(tokens + 1) + ". " + san;
    tokens += 2;
  }
  *out_len = h.size();
  if (out_cap < h.size() + 1) return out_cap ? DC_EINVAL : DC_SUCCESS;
  std::memcpy(out, h.c_str(), h.size() + 1);
  return DC_SUCCESS;
}


int dc_keccak256(const void* data, size_t len, uint8_t out[32]) {
  if ((!data && len) || !out) return DC_EINVAL;
  dc::Keccak256 k;
  k.update(data, len);
  k.final(out);
  return DC_SUCCESS;
}

int dc_state_hash_device(dc_ctx* c, const dc_pos* start, const char* history, const char* d_names,
                         const uint32_t* d_names_off, const uint16_t* d_moves, uint32_t n_games, uint32_t n_plies,
                         uint8_t* d_hashes) {
  ENTER_WORK(c);
  return state_hash_impl(c, start, history, d_names, d_names_off, d_moves, n_games, n_plies, d_hashes);
}

int dc_state_hash(dc_ctx* c, const dc_pos* start, const char* history, const char* names, const uint32_t* names_off,
                  const uint16_t* moves, uint32_t n_games, uint32_t n_plies, uint8_t* hashes) {
  ENTER_WORK(c);
  if ((n_games && n_plies && !moves) || (n_games && !hashes)) return DC_EINVAL;
  const size_t nm = (size_t)n_games * n_plies;
  HIP_TRY(c->moves.ensure(std::max<size_t>(nm, 1)));
  HIP_TRY(c->hashes.ensure(std::max<size_t>((size_t)32 * n_games, 1)));
  if (nm) HIP_TRY(hipMemcpyAsync(c->moves.p, moves, nm * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
  if (n_games) {
    if (!names || !names_off) return DC_EINVAL;
    const size_t n_off = (size_t)2 * n_games + 1;
    for (size_t i = 0; i + 1 < n_off; ++i)
      if (names_off[i + 1] < names_off[i]) return DC_EINVAL;
    const size_t raw = names_off[n_off - 1];
    HIP_TRY(c->names_raw.ensure(std::max<size_t>(raw, 1)));
    HIP_TRY(c->names_raw_off.ensure(n_off));
    if (raw) HIP_TRY(hipMemcpyAsync(c->names_raw.p, names, raw, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->names_raw_off.p, names_off, n_off * sizeof(u32), hipMemcpyHostToDevice, c->stream));
  }
  int r = state_hash_impl(c, start, history, c->names_raw.p, c->names_raw_off.p, c->moves.p, n_games, n_plies,
                          c->hashes.p);
  if (r != DC_SUCCESS) return r;
  if (n_games) HIP_TRY(hipMemcpyAsync(hashes, c->hashes.p, (size_t)32 * n_games, hipMemcpyDeviceToHost, c->stream));
  return sync_ctx(c);
}

// Test hook (not in the header): the state hash's pre-pass budget in bytes, so
// a test can force the hash kernel's own validation path and compare hashes.
extern "C" __attribute__((visibility("default"))) int dc_test_hash_prepass_max(dc_ctx* c, uint64_t bytes) {
  if (!c) return DC_EINVAL;
  c->hash_prepass_max = bytes;
  return DC_SUCCESS;
}

// Test hook (not in the header): the state hash's BCD move-number bound
// (clamped to 10^7), so a test can force the kernel's division path.
extern "C" __attribute__((visibility("default"))) int dc_test_hash_bcd_max(dc_ctx* c, uint32_t bound) {
  if (!c) return DC_EINVAL;
  c->hash_bcd_max = bound < 10000000u ? bound : 10000000u;
  return DC_SUCCESS;
}

int dc_gen_games_device(dc_ctx* c, uint32_t rules, uint64_t seed, uint64_t first_game, uint32_t n_games,
                        uint32_t n_plies, uint32_t noise_per_256, uint16_t* d_out) {
  ENTER_WORK(c);
  if (rules > DC_RULES_FIDE || (n_games && n_plies && !d_out) || noise_per_256 > 256) return DC_EINVAL;
  if (!n_games || !n_plies) return DC_SUCCESS;
  HIP_TRY(c->timed("gen_games", (u64)n_games * n_plies, [&] {
    return rules == DC_RULES_REF
               ? dc::launch_gen_games_ref(c->stream, seed, first_game, n_games, n_plies, noise_per_256, d_out)
               : dc::launch_gen_games_fide(c->stream, seed, first_game, n_games, n_plies, noise_per_256, d_out);
  }));
  return sync_ctx(c);
}

int dc_gen_games(dc_ctx* c, uint32_t rules, uint64_t seed, uint64_t first_game, uint32_t n_games, uint32_t n_plies,
                 uint32_t noise_per_256, uint16_t* out) {
  ENTER_WORK(c);
  if (rules > DC_RULES_FIDE || (n_games && n_plies && !out) || noise_per_256 > 256) return DC_EINVAL;
  const size_t nm = (size_t)n_games * n_plies;
  if (!nm) return DC_SUCCESS;
  HIP_TRY(c->moves.ensure(nm));
  int r = dc_gen_games_device(c, rules, seed, first_game, n_games, n_plies, noise_per_256, c->moves.p);
  if (r != DC_SUCCESS) return r;
  HIP_TRY(hipMemcpyAsync(out, c->moves.p, nm * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream));
  return sync_ctx(c);
}

}  // extern "C"
