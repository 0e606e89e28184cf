// dc_san_resolve.hip -- SAN tokens -> move words (include/dchess.h "notation
// input"), the inverse of k_replay_san's bytes + dc_san_format.
//
//   k_san_resolve   one lane per game; every ply is the same trip: read the
//                   token, find the side to move's pieces that fit it and may
//                   legally go to its target, write the move word (or a
//                   flagged word), make the move if there was exactly one
//   k_starts_san_resolve   the same lane body (san_resolve_lane<true>) from a start
//                   position per game, and the position each game reached
//
// Which piece "Nd2" means is a question of legality (pins, checks, en passant),
// so the trip runs the validator's analysis once (fpos + analyse) and asks
// fide_piece_targets for the few candidates that are left after the token's
// kind, its origin hints and the reverse geometry from the target (a knight's
// move, a line of the kind, a pawn's one or two origin squares) have narrowed
// them: almost always one piece.  No history, no clocks, no adjudication: a
// mated or stalemated side has no legal move, so its tokens find no match by
// themselves.
#include <hip/hip_runtime.h>

#include "dc_common.h"
#include "dc_san_resolve.h"

namespace dc {

namespace {

enum : u32 { MV_NONE = 0xFFFFu, MV_NOMATCH = 0x8001u, MV_AMBIGUOUS = 0x8002u, MV_MALFORMED = 0x8003u };
enum : u32 {
  TOK_NONE = 0xFFFFFFFFu,
  TOK_FILE_GIVEN = 1u << 12,
  TOK_RANK_GIVEN = 1u << 16,
  TOK_FIELDS = 0xFFFFFu,  // everything a castle token must leave 0
  TOK_RESERVED = 0xFE000000u
};

// kind > 5, promo > 4, reserved bits, both castle bits, a castle with other
// fields, a promotion on a piece
__device__ __forceinline__ bool token_malformed(u32 tok) {
  const u32 kind = (tok >> 6) & 7, promo = (tok >> 9) & 7, castle = (tok >> 20) & 3;
  return (tok & TOK_RESERVED) || kind > 5 || promo > 4 || castle == 3 || (castle && (tok & TOK_FIELDS)) ||
         (kind != 0 && promo != 0);
}

// The move word of a well-formed token, or MV_NOMATCH / MV_AMBIGUOUS.
template <int STM>
__device__ __forceinline__ u32 resolve_stm(const Board& b, u32 meta, u32 tok) {
  typedef FDir<STM> FD;
  const FPos<STM> f = fpos<STM>(b);
  const Analysis a = analyse<STM>(f);
  const u32 castle = (tok >> 20) & 3;
  if (castle) {
    // castle_targets holds a square only with the king at home, out of check
    const int t = FD::HOME + ((castle & 1) ? 2 : -2);
    const bool fit = (castle_targets<STM>(f, a, meta, b) >> t) & 1;
    return fit ? ((u32)FD::HOME | ((u32)t << 6)) : MV_NOMATCH;
  }
  const int t = (int)(tok & 63);
  const u32 kind = (tok >> 6) & 7, promo = (tok >> 9) & 7;
  const u64 tb = 1ull << t;
  u64 hint = ~0ull;
  if (tok & TOK_RANK_GIVEN) hint = 0xFFull << (8 * ((tok >> 17) & 7));
  u64 set, near;
  if (kind == 0) {
    // a pawn stands on the origin file, or on the target's file if none is
    // written: "e4" is the push, "dxe4" the capture
    const bool last = (tb & FD::LAST) != 0;
    if (last ? (promo == 0) : (promo != 0)) return MV_NOMATCH;
    const u32 file = (tok & TOK_FILE_GIVEN) ? ((tok >> 13) & 7) : (u32)(t & 7);
    set = f.P & (kFileA << file);
    near = file == (u32)(t & 7) ? (sh<-FD::F>(tb) | sh<-2 * FD::F>(tb)) : pawn_attacks<1 - STM>(tb);
  } else {
    if (tok & TOK_FILE_GIVEN) hint &= kFileA << ((tok >> 13) & 7);
    const Lines l = lines_of(t);
    const u64 q = f.O & f.D;
    const u64 orth = l.file | l.rank, diag = l.diag | l.anti;
    set = kind == 1 ? f.N : kind == 2 ? (f.D & ~q) : kind == 3 ? (f.O & ~q) : kind == 4 ? q : f.K;
    // a king one step away: a K token never means a castle
    near = kind == 1   ? knight_attacks(tb)
           : kind == 2 ? diag
           : kind == 3 ? orth
           : kind == 4 ? (orth | diag)
                       : king_attacks(tb);
  }
  u64 cand = set & near & hint;
  u32 fits = 0, from = 0;
  while (cand) {
    const int s = lsb(cand);
    cand &= cand - 1;
    const u64 targets = fide_piece_targets<STM>(b, meta, f, a, s);
    const u32 fit = (u32)(targets >> t) & 1u;
    fits += fit;
    from = fit ? (u32)s : from;
  }
  return fits == 0 ? MV_NOMATCH : fits > 1 ? MV_AMBIGUOUS : (from | ((u32)t << 6) | (promo << 12));
}

// One lane's game.  STARTS: the game's own start position (starts, may be null:
// the shared start) and, after the loop, the position after its last resolved
// move (finals, may be null).  Otherwise the two pointers are not looked at.
template <bool STARTS>
__device__ __forceinline__ void san_resolve_lane(Board start, u32 stm0, u32 meta0, const DevPos* __restrict__ starts,
                                                 DevPos* __restrict__ finals, const u32* __restrict__ tokens,
                                                 u32 n_games, u32 n_plies, uint16_t* __restrict__ moves,
                                                 u32* __restrict__ first_bad, u64* __restrict__ counts) {
  const u64 g = (u64)blockIdx.x * kResolveBlock + threadIdx.x;
  const bool active = g < n_games;
  Board b = start;
  u32 stm = stm0, meta = meta0;
  if (STARTS && active && starts) load_start(starts, g, b, stm, meta);
  u32 bad_at = n_plies;
  u32 n_tok = 0, n_ok = 0, n_nomatch = 0, n_ambiguous = 0, n_malformed = 0;
  for (u32 ply = 0; ply < n_plies; ++ply) {
    const size_t at = (size_t)ply * n_games + g;
    const u32 tok = active ? tokens[at] : TOK_NONE;
    u32 word = MV_NONE;
    if (tok != TOK_NONE) {
      ++n_tok;
      word = token_malformed(tok) ? MV_MALFORMED : stm ? resolve_stm<1>(b, meta, tok) : resolve_stm<0>(b, meta, tok);
      const bool ok = (word & 0x8000u) == 0;
      if (ok) {
        meta = fide_make_rt(b, stm, meta, (int)(word & 63), (int)((word >> 6) & 63), (int)((word >> 12) & 7));
        stm ^= 1;
      }
      n_ok += ok ? 1u : 0u;
      n_nomatch += word == MV_NOMATCH ? 1u : 0u;
      n_ambiguous += word == MV_AMBIGUOUS ? 1u : 0u;
      n_malformed += word == MV_MALFORMED ? 1u : 0u;
      bad_at = (!ok && bad_at == n_plies) ? ply : bad_at;
    }
    // one store a trip and a whole row segment a wave
    if (active) moves[at] = (uint16_t)word;
  }
  if (active && first_bad) first_bad[g] = bad_at;
  if (STARTS && active && finals) store_final(finals, g, b, stm, meta);
  if (counts) {
    // integers: the order of the waves' adds does not matter
    const u64 s0 = wave_sum64(n_tok), s1 = wave_sum64(n_ok), s2 = wave_sum64(n_nomatch), s3 = wave_sum64(n_ambiguous),
              s4 = wave_sum64(n_malformed);
    if (lane_id() == 0) {
      atomicAdd((unsigned long long*)&counts[0], (unsigned long long)s0);
      atomicAdd((unsigned long long*)&counts[1], (unsigned long long)s1);
      atomicAdd((unsigned long long*)&counts[2], (unsigned long long)s2);
      atomicAdd((unsigned long long*)&counts[3], (unsigned long long)s3);
      atomicAdd((unsigned long long*)&counts[4], (unsigned long long)s4);
    }
  }
}

}  // namespace

__global__ __launch_bounds__(kResolveBlock) void k_san_resolve(Board start, u32 stm0, u32 meta0,
                                                               const u32* __restrict__ tokens, u32 n_games,
                                                               u32 n_plies, uint16_t* __restrict__ moves,
                                                               u32* __restrict__ first_bad, u64* __restrict__ counts) {
  san_resolve_lane<false>(start, stm0, meta0, nullptr, nullptr, tokens, n_games, n_plies, moves, first_bad, counts);
}

__global__ __launch_bounds__(kResolveBlock) void k_starts_san_resolve(
    Board start, u32 stm0, u32 meta0, const DevPos* __restrict__ starts, DevPos* __restrict__ finals,
    const u32* __restrict__ tokens, u32 n_games, u32 n_plies, uint16_t* __restrict__ moves,
    u32* __restrict__ first_bad, u64* __restrict__ counts) {
  san_resolve_lane<true>(start, stm0, meta0, starts, finals, tokens, n_games, n_plies, moves, first_bad, counts);
}

hipError_t launch_san_resolve(hipStream_t st, const DevPos& start, bool per_game, const DevPos* starts, DevPos* finals,
                              const u32* tokens, u32 n_games, u32 n_plies, uint16_t* moves, u32* first_bad,
                              u64* counts) {
  if (n_games == 0) return hipSuccess;
  if (n_plies && (!tokens || !moves)) return hipErrorInvalidValue;
  const dim3 grid(blocks_for(n_games, kResolveBlock)), block(kResolveBlock);
  const Board b{start.bb[0], start.bb[1], start.bb[2], start.bb[3]};
  const u32 stm = start.stm & 1, meta = pack_meta(start.castle, start.ep);
  if (per_game)
    hipLaunchKernelGGL(k_starts_san_resolve, grid, block, 0, st, b, stm, meta, starts, finals, tokens, n_games,
                       n_plies, moves, first_bad, counts);
  else
    hipLaunchKernelGGL(k_san_resolve, grid, block, 0, st, b, stm, meta, tokens, n_games, n_plies, moves, first_bad,
                       counts);
  return hipGetLastError();
}

}  // namespace dc
