// dc_perft_stats.hip -- the final stage of dc_perft_stats: every move of every
// frontier node (ply depth - 1) classified into the DC_PS_* counters.
//
// The frontier is built by the level pipeline of dc_perft.hip (k_expand_top,
// k_level_count, k_chunk_scan, k_level_write); this unit holds only k_leaf_stats
// and its launch wrapper, so the perft kernels' device code is untouched.
//
// Shape (wave-level: k_count2b's LDS compaction with a wave, not a block, as
// the unit): a wave stages 64 parents in LDS, compacts their legal
// moves into LDS slots at wave-scan offsets (windows of kLsCap slots), and then
// every lane takes one (parent, move) slot per round, so the lanes stay full
// whatever the parents' branching.  For its slot a lane reads the move's flags
// from the parent (target occupied, en passant, castle, promotion, the victim's
// kind), makes the child, and under FIDE counts the child's legal moves with
// the analysis' checkers (fide_count_checkers): check, double and discovered
// check follow from the checkers, mate and stalemate from a count of zero.
// Counters accumulate per root tag in LDS (kPsCount histograms of 256 u64,
// 22 KB), one LDS atomic per wave, counter and round when the round's slots
// share a root tag (the norm: nodes stay ordered by root move), and are flushed
// once per block with vector atomics.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/dchess.h"
#include "dc_common.h"
#include "dc_launch.h"
#include "dc_perft.h"

namespace dc {

static_assert(kPsCount == DC_PS_COUNT, "dchess.h perft statistics");

namespace {

// The rules policies of this stage (named so that the spill-free check, which
// covers every kernel instantiated over a *FideRules / *RefRules type, covers it).
struct StatsRefRules {
  static constexpr bool kMeta = false;
  static constexpr int kMinBlocks = 3;
};
struct StatsFideRules {
  static constexpr bool kMeta = true;
  static constexpr int kMinBlocks = 3;
};

constexpr u32 kLsWaves = 4;
constexpr u32 kLsCap = 64 * 24;  // move slots per wave and window (startpos ply-4 parents average 25 moves)

struct LsShared {
  u64 hist[kPsCount][256];
  Board par[kLsWaves][64];
  uint16_t pmeta[kLsWaves][64];
  uint16_t ptag[kLsWaves][64];
  uint16_t move[kLsWaves][kLsCap];
  uint8_t owner[kLsWaves][kLsCap];  // the slot's parent (lane)
};
static_assert(3 * sizeof(LsShared) <= 160 * 1024, "three blocks per CU");

// The counters one move adds to, as a bit mask over DC_PS_*.
// p: the parent (side STM to move), pm its meta; f, t, promo: a legal move.
template <class R, int STM>
__device__ __forceinline__ u32 classify(const Board& p, u32 pm, int f, int t, int promo) {
  u32 fl = 1u << DC_PS_NODES;
  const u32 victim = nibble(p, t) >> 1;
  if constexpr (!R::kMeta) {
    if (victim) fl |= 1u << DC_PS_CAPTURES;
    if (victim == KC_K) fl |= 1u << DC_PS_KING_CAPTURES;
    return fl;
  } else {
    const u32 kind = nibble(p, f) >> 1;
    const bool ep = kind == KC_P && t == meta_ep(pm);
    const bool castle = kind == KC_K && (t - f == 2 || f - t == 2);
    if (victim || ep) fl |= 1u << DC_PS_CAPTURES;
    if (ep) fl |= 1u << DC_PS_EP;
    if (castle) fl |= 1u << DC_PS_CASTLES;
    if (promo) fl |= 1u << DC_PS_PROMOTIONS;
    Board ch = p;
    const u32 cm = fide_make<STM>(ch, pm, f, t, promo);
    u64 chk;
    const u32 replies = fide_count_checkers<1 - STM>(ch, cm, chk);
    if (chk) {
      fl |= 1u << DC_PS_CHECKS;
      if (chk & (chk - 1)) {
        fl |= 1u << DC_PS_DOUBLE;
      } else {
        // one checker that is not the piece that moved (on t; a castle's rook
        // lands between f and t): a discovered check
        const int cs = lsb(chk);
        if (cs != t && !(castle && cs == ((f + t) >> 1))) fl |= 1u << DC_PS_DISCOVERED;
      }
      if (replies == 0) fl |= 1u << DC_PS_CHECKMATES;
    } else if (replies == 0) {
      fl |= 1u << DC_PS_STALEMATES;
    }
    return fl;
  }
}

template <class R, int STM>
__global__ __launch_bounds__(64 * kLsWaves, R::kMinBlocks) void k_leaf_stats(
    const Board* __restrict__ nodes, const uint16_t* __restrict__ meta, const uint16_t* __restrict__ tags,
    const Range* __restrict__ rng, const PerftResult* __restrict__ res, u32 root, u64* __restrict__ stats) {
  __shared__ LsShared sh;
  for (u32 k = threadIdx.x; k < kPsCount * 256; k += 64 * kLsWaves) (&sh.hist[0][0])[k] = 0;
  __syncthreads();
  const u32 w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const u32 lane = lane_id();
  Board* par = sh.par[w];
  uint16_t* pmeta = sh.pmeta[w];
  uint16_t* ptag = sh.ptag[w];
  uint16_t* move = sh.move[w];
  uint8_t* owner = sh.owner[w];
  const u64 lo = root ? 0 : rng->lo, hi = root ? 1 : rng->hi;  // (the root: one node, no Range)
  const u64 groups = (hi - lo + 63) >> 6;
  for (u64 g = (u64)blockIdx.x * kLsWaves + w; g < groups; g += (u64)gridDim.x * kLsWaves) {  // wave-uniform
    const u64 i = lo + (g << 6) + lane;
    const bool valid = i < hi;
    Board p{0, 0, 0, 0};
    u32 pm = 0, tag = 0;
    if (valid) {
      p = load_board(nodes, i);
      if constexpr (R::kMeta) pm = meta[i];
      tag = root ? 0u : tags[i];
    }
    u32 cnt = 0;
    if (valid) {
      if constexpr (R::kMeta) cnt = fide_count<STM>(p, pm);
      else cnt = ref_count<STM>(p);
    }
    const u32 incl = wave_incl_scan(cnt);
    const u32 excl = incl - cnt;
    const u32 total = lane_bcast(incl, 63);
    par[lane] = p;
    pmeta[lane] = (uint16_t)pm;
    ptag[lane] = (uint16_t)tag;
    for (u32 base = 0; base < total; base += kLsCap) {
      wave_lds_sync();  // the parents are staged; the previous window's slots are consumed
      if (valid && excl < base + kLsCap && excl + cnt > base) {
        // the parent read back from LDS: p is not live across the slot rounds
        const Board pp = par[lane];
        u32 j = excl - base;  // slot index in this window (wraps below 0 for earlier windows)
        auto put = [&](int f, int t, int promo) {
          if (j < kLsCap) {
            move[j] = (uint16_t)((u32)f | ((u32)t << 6) | ((u32)promo << 12));
            owner[j] = (uint8_t)lane;
          }
          ++j;
        };
        if constexpr (R::kMeta) fide_for_each_move<STM>(pp, (u32)pmeta[lane], put);
        else ref_for_each_move<STM>(pp, [&](int f, int t) { put(f, t, 0); });
      }
      wave_lds_sync();
      const u32 nslots = min(kLsCap, total - base);
      for (u32 r0 = 0; r0 < nslots; r0 += 64) {  // wave-uniform
        const u32 r = r0 + lane;
        const bool live = r < nslots;
        u32 fl = 0, tg = 0;
        if (live) {
          const u32 e = move[r];
          const u32 pl = owner[r];
          fl = classify<R, STM>(par[pl], pmeta[pl], (int)(e & 63), (int)((e >> 6) & 63), (int)((e >> 12) & 7));
          tg = ptag[pl];
          if (root) {  // depth 1: the tag is the move's place among the root moves
            const u32 nr = min(res->n_root, 256u);
            for (u32 k = 0; k < nr; ++k)
              if (res->root_moves[k] == e) tg = k;
          }
        }
        const u64 lm = ballot(live);
        const u32 tg0 = lane_bcast(tg, (u32)lsb(lm));  // (r0 < nslots: lane 0 is live)
        const bool uni = ballot(live && tg != tg0) == 0;
#pragma unroll
        for (u32 k = 0; k < kPsCount; ++k) {
          const u64 m = ballot((fl >> k) & 1u);
          if (uni) {
            if (m != 0 && lane == (u32)lsb(m))
              atomicAdd((unsigned long long*)&sh.hist[k][tg0], (unsigned long long)pc(m));
          } else if ((fl >> k) & 1u) {
            atomicAdd((unsigned long long*)&sh.hist[k][tg], 1ull);
          }
        }
      }
    }
    wave_lds_sync();  // par / ptag are rewritten by the next group
  }
  __syncthreads();
  for (u32 k = threadIdx.x; k < kPsCount * 256; k += 64 * kLsWaves) {
    const u32 tg = k & 255u, ctr = k >> 8;
    const u64 v = sh.hist[ctr][tg];
    if (v) atomicAdd((unsigned long long*)(stats + (size_t)tg * kPsCount + ctr), (unsigned long long)v);
  }
}

}  // namespace

hipError_t launch_leaf_stats(hipStream_t st, u32 rules, int stm, const Board* nodes, const uint16_t* meta,
                             const uint16_t* tags, const Range* rng, u64 n_bound, const PerftResult* res, u32 root,
                             u64* stats) {
  // one resident wave of blocks at most (the kernel strides over the groups)
  constexpr u32 kBlock = 64 * kLsWaves;
  const u32 want = (u32)std::min<u64>(std::max<u64>(1, (n_bound + kBlock - 1) / kBlock), 0xFFFFFFFFull);
  with_rules<StatsRefRules, StatsFideRules>(rules, [&](auto R) {
    with_stm(stm, [&](auto S) {
      launch_resident(k_leaf_stats<tagged<decltype(R)>, S()>, kBlock, want, st, nodes, meta, tags, rng, res, root,
                      stats);
    });
  });
  return hipGetLastError();
}

}  // namespace dc
