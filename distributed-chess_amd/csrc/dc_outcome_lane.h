// dc_outcome_lane.h -- the adjudicating replay of one lane, device only: the one
// loop behind k_replay_outcome / k_starts_replay_outcome (dc_outcome.hip) and
// k_replay_san / k_starts_replay_san (dc_san.hip).  The history layout is
// described in dc_outcome.hip, the SAN byte in dc_san.hip.
#pragma once
#include "dc_common.h"
#include "dc_outcome.h"

namespace dc {

enum : u32 { GO_ONGOING = 0, GO_WHITE_WINS, GO_BLACK_WINS, GO_STALEMATE, GO_DEAD, GO_FIVEFOLD, GO_SEVENTYFIVE };
constexpr u32 kClockEnd = kOutcomeSlots - 1;  // 150 half-moves: the 75-move rule
enum : u32 { SAN_CAPTURE = 8, SAN_FILE = 16, SAN_RANK = 32, SAN_CHECK = 64, SAN_MATE = 128, SAN_NONE = 0xFF };

__device__ __forceinline__ u64* key_at(u64* hist, u32 slot, u32 stride, u32 lane_game) {
  return hist + (size_t)slot * kOutcomeKeyWords * stride + lane_game;
}

// fide_verdict_stm (dc_fide_rules.h) == V_OK, and for an accepted move the low
// six bits of its SAN byte.  Disambiguation (FIDE C.10.3): `others` = the other
// pieces of the mover's kind and colour that attack t (a reverse attack from t)
// and may legally go there.  The played move is legal, so t is not ours and,
// in check, t resolves the check: an unpinned attacker of t is legal.  A pinned
// one is legal only out of check and along its pin line, i.e. when it stands on
// the line through the king and t.
template <int STM>
__device__ __forceinline__ bool san_verdict_stm(const Board& b, u32 meta, u32 m, u32& low) {
  typedef FDir<STM> FD;
  const int s = (int)(m & 63), t = (int)((m >> 6) & 63);
  const u32 promo = (m >> 12) & 7;
  const FPos<STM> f = fpos<STM>(b);
  const Analysis a = analyse<STM>(f);
  const u64 targets = fide_piece_targets<STM>(b, meta, f, a, s);
  if (!((targets >> t) & 1)) return false;
  const u64 from = 1ull << s;
  const bool pawn = (from & f.P) != 0;
  const bool is_promo = pawn && ((1ull << t) & FD::LAST);
  if (is_promo ? (promo < 1 || promo > 4) : (promo != 0)) return false;
  const u64 q = f.O & f.D;
  const bool orth = (from & f.O) != 0, diag = (from & f.D) != 0;
  const u32 kind = pawn ? 0u : (from & f.N) ? 1u : (from & f.K) ? 5u : (orth && diag) ? 4u : orth ? 3u : 2u;
  const u64 same = ((from & f.N) ? f.N : (orth && diag) ? q : orth ? (f.O & ~q) : diag ? (f.D & ~q) : 0ull) & ~from;
  u32 flags = ((f.occ >> t) & 1) || (pawn && t == meta_ep(meta)) ? SAN_CAPTURE : 0u;
  // the pieces of the kind that stand a knight's move from t, or on a line of their kind through
  // t: rare, so the blockers are looked at only for those
  const Lines l = lines_of(t);
  const u64 near = (from & f.N) ? knight_attacks(1ull << t)
                                : ((orth ? (l.file | l.rank) : 0ull) | (diag ? (l.diag | l.anti) : 0ull));
  if (same & near) {
    u64 att = (from & f.N) ? near : 0ull;
    if (orth) att |= line_attacks(t, l.file, f.occ) | line_attacks(t, l.rank, f.occ);
    if (diag) att |= line_attacks(t, l.diag, f.occ) | line_attacks(t, l.anti, f.occ);
    const u64 along = (a.checkers || a.ksq < 0) ? 0ull : line_through(a.ksq, t);
    const u64 others = att & same & (~a.pinned | along);
    if (others) {
      const bool on_file = (others & (kFileA << (s & 7))) != 0;
      const bool on_rank = (others & (0xFFull << (s & 56))) != 0;
      flags |= !on_file ? SAN_FILE : !on_rank ? SAN_RANK : (SAN_FILE | SAN_RANK);
    }
  }
  low = kind | flags;
  return true;
}

// fide_verdict's gates (out of range, no piece, wrong turn), then the above.
__device__ __forceinline__ bool san_verdict(const Board& b, u32 stm, u32 meta, u32 m, u32& low) {
  if (m & 0x8000u) return false;
  const u32 nib = nibble(b, (int)(m & 63));
  if ((nib >> 1) == 0 || (nib & 1) != stm) return false;
  return stm ? san_verdict_stm<1>(b, meta, m, low) : san_verdict_stm<0>(b, meta, m, low);
}

// The block's record (kOutcomeRecord words, dc_outcome.h) from its lanes' counts,
// digests d (0 for an inactive lane) and results; k_outcome_reduce combines them.
__device__ __forceinline__ void store_block_record(u32 first, bool active, u32 result, u32 validated, u32 accepted,
                                                   u64 d, u64* __restrict__ partial) {
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

// The adjudicating replay of one lane.  STARTS: the game's own start position
// and clock (starts / clocks, either may be null: the shared start, the shared
// clock) and, after the loop, the position it stopped in (finals, may be null);
// all three indexed by the game, not by the chunk's lane.  Otherwise the shared
// start alone, and the three pointers are not looked at.  SAN: also the SAN
// byte of every ply into san; otherwise san is not looked at.
template <bool STARTS, bool SAN>
__device__ __forceinline__ void replay_adjudicate_lane(Board start, u32 stm0, u32 meta0, u32 clock0,
                                                       const DevPos* __restrict__ starts,
                                                       const uint16_t* __restrict__ clocks,
                                                       DevPos* __restrict__ finals, const uint16_t* __restrict__ moves,
                                                       u32 n_games, u32 n_plies, u32 first, u32 count, u64* hist,
                                                       u32 stride, u64* __restrict__ outcomes,
                                                       uint8_t* __restrict__ san, u64* __restrict__ bitmap,
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
  // SAN only.  Both out here: a variable of the loop's body, even a dead one, has to be ended on
  // each exit of the loop, which changes k_replay_outcome's code ("One lane body").
  [[maybe_unused]] u32 low = 0;  // kind | capture | file | rank of the last accepted move (ply consumed - 1)
  [[maybe_unused]] u32 byte;     // the whole byte of ply - 1
  bool fresh = active;           // the position has not been adjudicated yet
  u32 ply = 0;
  for (;; ++ply) {
    if constexpr (SAN) byte = SAN_NONE;  // no move unless this trip adjudicates what it led to
    if (fresh) {
      fresh = false;
      u64 checkers;
      const u32 n_legal = stm ? fide_count_checkers<1>(b, meta, checkers) : fide_count_checkers<0>(b, meta, checkers);
      // the move that led here is complete now: it gives check, it mates
      if constexpr (SAN) byte = low | (checkers ? SAN_CHECK : 0u) | (checkers && n_legal == 0 ? SAN_MATE : 0u);
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
        u64* k = key_at(hist, clock, stride, local);
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
    // one store a trip and a whole row segment a wave: the byte of the ply before
    if constexpr (SAN)
      if (active && ply) san[(size_t)(ply - 1) * n_games + g] = (uint8_t)byte;
    if (ply >= n_plies) break;
    const bool live = active && result == GO_ONGOING;
    if (ballot(live) == 0) break;  // every game of the wave has ended (a ballot is wave-uniform)
    const u32 m = live ? moves[(size_t)ply * n_games + g] : 0xFFFFu;
    bool ok = false;
    if (m != 0xFFFFu) {
      ++validated;
      if constexpr (SAN) ok = san_verdict(b, stm, meta, m, low);
      else ok = fide_verdict(b, stm, meta, m) == V_OK;
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
  // the plies no game of the wave reached: no SAN, accept bits 0
  if constexpr (SAN)
    if (active)
      for (u32 p = ply; p < n_plies; ++p) san[(size_t)p * n_games + g] = (uint8_t)SAN_NONE;
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
  store_block_record(first, active, result, validated, accepted, d, partial);
}

}  // namespace dc
