// dc_api_perft.hip -- the perft driver: dc_perft, dc_perft_shard,
// dc_perft_batch and the *_repeat_device forms, with their captured graphs;
// dc_perft_stats and dc_perft_stats_shard (the plain enqueue path only).
#include <cstring>

#include "dc_ctx.h"
#include "dc_fide.h"  // pack_meta

// =================================================================== perft
// Device-driven level pipeline (dc_perft.hip): the level sizes live in device
// Range descriptors, capacities are bounded on the host (n_bound x 64 children,
// within kSpecBudget bytes per level), and the host synchronises once at the
// end.  Writes past a capacity are dropped and flagged; the run is then
// repeated in exact mode, which reads every level size back before sizing the
// next (one sync per level).  Level order is deterministic, so ranks that
// rebuild the top levels agree on the frontier and on each one's shard of it.
namespace {

constexpr u64 kBranchBound = 64;                    // speculative children per node
constexpr u64 kSpecBudget = 16ull << 30;            // bytes per speculative level (of 288 GB HBM)
constexpr u64 kNodeBytes = sizeof(Board) + 2 * sizeof(uint16_t);
// Deepest BFS level under REF: below it, K4 (k_perft_dfs) walks per lane.
// Ply 5 of startpos is 4.9M nodes (196 MB); a typical middlegame ply 5 stays
// within the speculative budget (Kiwipete's is 193M nodes, 6.6 GB).
constexpr u32 kDfsFrontier = 5;
// REF perft(8) takes the fused final stage from ply 5 instead (k_level_moves
// + k_count3c with 64-bit move words: startpos ply 6 is 120M words, 0.96 GB)
// while the words fit this capacity; a larger ply 6 (or DCHESS_PERFT_K4=1 in
// the environment, for tests) goes through K4 from ply 5.  REF perft(9) builds
// ply 6 as boards (startpos: 120M, 4.3 GB) and runs the fused stage over
// slices of kSliceNodes grandparents (each slice's words fit the capacity:
// 2^21 nodes x 256 moves); a ply 6 past kWideLevelBytes goes through K4.
constexpr u64 kWideWordsMax = 1ull << 29;  // 4.3 GB of words
constexpr u64 kSliceNodes = 1ull << 21;
constexpr u64 kWideLevelBytes = 48ull << 30;
// (DCHESS_PERFT_WIDE_MAX lowers it, so a test can take the fallback on a small tree)
u64 wide_words_max() {
  const char* e = std::getenv("DCHESS_PERFT_WIDE_MAX");
  const u64 v = e ? std::strtoull(e, nullptr, 10) : 0;
  return v ? std::min<u64>(v, kWideWordsMax) : kWideWordsMax;
}
// (DCHESS_PERFT_WIDE_LEVEL_MAX lowers kWideLevelBytes the same way)
u64 wide_level_bytes() {
  const char* e = std::getenv("DCHESS_PERFT_WIDE_LEVEL_MAX");
  const u64 v = e ? std::strtoull(e, nullptr, 10) : 0;
  return v ? std::min<u64>(v, kWideLevelBytes) : kWideLevelBytes;
}
bool perft_k4_forced() {
  const char* e = std::getenv("DCHESS_PERFT_K4");
  return e && e[0] == '1';
}

int ensure_level(dc_ctx* c, int b, u64 n, bool fide) {
  const size_t want = std::max<u64>(n, 1);
  HIP_TRY(c->nodes[b].ensure(want));
  HIP_TRY(c->tags[b].ensure(want));
  if (fide) HIP_TRY(c->meta[b].ensure(want));
  return DC_SUCCESS;
}

int read_range(dc_ctx* c, int level, u64* n) {
  dc::Range r;
  HIP_TRY(hipMemcpyAsync(&r, c->rng.p + level, sizeof r, hipMemcpyDeviceToHost, c->stream));
  int e = sync_ctx(c);
  if (e != DC_SUCCESS) return e;
  *n = r.hi - r.lo;
  return DC_SUCCESS;
}

// The experiment knob of this driver (A/B build only: the product reads none,
// see ab_env), read once per process.
struct Knobs {
  // Which k_front shapes deduplicate their grandparents (DESIGN.md section 3.9:
  // decided by measurement).  A mask: 1 perft(7) unsharded, 2 perft(7) shards,
  // 4 perft(6) unsharded, 8 perft(6) shards.
  u32 front_dedup = (u32)dc::ab_int("DC_FRONT_DEDUP", 1, 0);
};
const Knobs& knobs() {
  static const Knobs k;
  return k;
}

// One perft request, as the C ABI states it.
struct PerftReq {
  uint32_t rules;
  const dc_pos* pos;
  u32 n_pos;  // root positions expanded together (dc_perft_batch; 1 otherwise)
  uint32_t depth, split_depth, shard, n_shards;
  bool fide() const { return rules == DC_RULES_FIDE; }
  bool sharded() const { return n_shards > 1; }
};

// Writes *pos into the pinned root staging block.  Copies already queued on
// the stream (dc_perft_repeat_device returns with runs in flight, each reading
// the block when it executes) must see the value they were queued with, so a
// changed root first waits for the stream.  A capture only ever re-stages the
// root of the run that was just synchronised (the value is unchanged).
bool root_staged(const dc_ctx* c, const dc_pos* pos, u32 n) {
  if (c->root_host->n != n) return false;
  for (u32 i = 0; i < n; ++i) {
    const Board rb{pos[i].bb[0], pos[i].bb[1], pos[i].bb[2], pos[i].bb[3]};
    if (std::memcmp(&c->root_host->b[i], &rb, sizeof(Board)) != 0 ||
        c->root_host->meta[i] != dc::pack_meta(pos[i].castle, pos[i].ep))
      return false;
  }
  return true;
}

int write_root_host(dc_ctx* c, const dc_pos* pos, u32 n) {
  if (root_staged(c, pos, n)) return DC_SUCCESS;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  HIP_TRY(hipStreamIsCapturing(c->stream, &cs));
  if (cs != hipStreamCaptureStatusNone) return DC_EHIP;  // unreachable: captures follow a synchronised run
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (u32 i = 0; i < n; ++i) {
    c->root_host->b[i] = Board{pos[i].bb[0], pos[i].bb[1], pos[i].bb[2], pos[i].bb[3]};
    c->root_host->meta[i] = dc::pack_meta(pos[i].castle, pos[i].ep);
  }
  c->root_host->n = n;
  return DC_SUCCESS;
}

// the staged roots to the device root arrays (stream-ordered)
int upload_roots(dc_ctx* c, u32 n, bool meta) {
  HIP_TRY(hipMemcpyAsync(c->root.p, c->root_host->b, n * sizeof(Board), hipMemcpyHostToDevice, c->stream));
  if (meta)  // (REF reads no castle / ep: one graph node less per run)
    HIP_TRY(hipMemcpyAsync(c->root_meta.p, c->root_host->meta, n * sizeof(uint16_t), hipMemcpyHostToDevice,
                           c->stream));
  return DC_SUCCESS;
}

// The shape of one perft's launch sequence: which levels are built how, decided
// from the request and the knobs alone (no context, no allocation).
struct PerftShape {
  u32 F;            // level handed to the final stage
  u32 T;            // plies built by the single-workgroup top kernel
  u32 S;            // the level a sharded run is cut at
  u32 Ldfs;         // plies K4 walks per lane above the final stage (more than 3: unsupported)
  int final_plies;  // depth 1: no final stage
  bool wide;        // REF perft(8) and (9): 64-bit move words below ply 5 or slices of ply 6 (see kWideWordsMax)
  bool sliced;
  bool fused3;
  bool shard_words;
  bool top_words;
  u64 cap_T;  // capacity of level T
};
constexpr u64 kTopCap[4] = {1, 256, 256 * 256, 1ull << 20};

// split_depth, within [1, F]
static u32 shard_level(u32 split_depth, u32 F) { return std::max<u32>(1, std::min(split_depth, F)); }

// Plies the single-workgroup top kernel builds, of `deepest` built in all (S: the
// level a sharded run is cut at).
static u32 top_plies(bool fide, bool exact, u32 deepest, bool sharded, u32 S) {
  u32 T = exact ? 1 : std::min<u32>(deepest, 3);
  // FIDE with ply 3 the deepest (perft depth 5): that ply (Kiwipete: 97,862
  // nodes) made inside the one workgroup was ~0.3 ms per position (rocprofv3,
  // round 4); stopping the top kernel one ply short leaves it to the level
  // kernels on every CU
  if (fide && !exact && T == deepest && deepest == 3) T = deepest - 1;
  return sharded ? std::min(T, S) : T;
}

static PerftShape perft_shape(const PerftReq& q, bool exact) {
  const bool fide = q.fide(), sharded = q.sharded();
  const uint32_t depth = q.depth, split_depth = q.split_depth;
  PerftShape s{};
  s.F = depth >= 3 ? depth - 2 : 1;
  s.wide = !fide && (depth == kDfsFrontier + 3 || depth == kDfsFrontier + 4) && !perft_k4_forced();
  s.sliced = s.wide && depth == kDfsFrontier + 4;
  // REF beyond ply kDfsFrontier: K4 walks the last Ldfs plies above the final
  // stage per lane (k_perft_dfs) instead of materialising those levels
  if (!fide && depth >= 3 && s.F > kDfsFrontier && !s.wide) {
    s.Ldfs = s.F - kDfsFrontier;
    s.F = kDfsFrontier;
  }
  s.final_plies = depth >= 3 ? 2 : 1;
  s.S = shard_level(split_depth, s.F);
  s.T = top_plies(fide, exact, s.F, sharded, s.S);
  s.cap_T = kTopCap[s.T];
  // REF final stage over the last three plies (k_count3c): the level F is
  // never written; its parents' level is counted and scanned, then expanded
  // group by group inside the final stage.  Needs a level to expand (L < F)
  // that is not the shard level.
  s.fused3 = !fide && s.Ldfs == 0 && s.final_plies == 2 && s.T < s.F && !(sharded && s.S == s.F);
  // The target ply of k_expand_top is made on many CUs by k_make_count (it
  // replaces that level's k_level_count) when that level is counted next.
  // A rank's strided shard of that ply (round 5): the words stay whole and
  // k_make_count makes only this rank's (word shard + i x n_shards), instead
  // of the one workgroup making the whole ply as boards and k_gather_shard
  // copying the shard out of it.
  s.shard_words = !exact && sharded && s.S == s.T && s.T >= 2 && s.T < s.F;
  s.top_words = !exact && s.T >= 2 && s.T < s.F && (!(sharded && s.S == s.T) || s.shard_words);
  return s;
}

// REF perft(6) / perft(7) of one root, unsharded or a strided shard of ply 3:
// the one-launch front end (k_front) + k_count3c.
static bool front_eligible(const PerftReq& q) {
  if (q.rules != DC_RULES_REF || q.n_pos != 1 || (q.depth != 6 && q.depth != 7)) return false;
  return !q.sharded() || perft_shape(q, false).S == 3;
}

// The buffers every perft sequence needs, allocated before anything is enqueued.
static int perft_ensure_common(dc_ctx* c) {
  if (!c->res_host) HIP_TRY(c->res_host.alloc());
  if (!c->root_host) {
    HIP_TRY(c->root_host.alloc());
    c->root_host->n = 0;
  }
  HIP_TRY(c->res.ensure(1));
  HIP_TRY(c->rng.ensure(16));
  HIP_TRY(c->root.ensure(dc::kMaxPerftRoots));
  HIP_TRY(c->root_meta.ensure(dc::kMaxPerftRoots));
  return DC_SUCCESS;
}

// k_front's sequence: the root upload (stage_root), k_front, k_count3c (and,
// where the grandparents are deduplicated, k_front_fold).
static int front_enqueue_seq(dc_ctx* c, const PerftReq& q, bool stage_root) {
  const dc_pos* pos = q.pos;
  const uint32_t depth = q.depth, shard = q.shard, n_shards = q.n_shards;
  int e = perft_ensure_common(c);
  if (e != DC_SUCCESS) return e;
  HIP_TRY(c->front_st.ensure(sizeof(dc::FrontState)));
  dc::FrontState* fst = reinterpret_cast<dc::FrontState*>(c->front_st.p);
  if (c->front_st_zeroed != c->front_st.p) {  // a new state block (stream-ordered before its first use)
    HIP_TRY(hipMemsetAsync(c->front_st.p, 0, sizeof(dc::FrontState), c->stream));
    c->front_st_zeroed = c->front_st.p;
  }
  // the grandparents' index is a move word's upper 20 bits
  const u32 cap_b = (u32)dc::kMoveWordNodesMax;
  const u64 cap_w = std::min<u64>((u64)cap_b * kBranchBound, 0xFFFFFFFFull);
  e = ensure_level(c, 0, cap_b, false);
  if (e != DC_SUCCESS) return e;
  HIP_TRY(c->move_words.ensure(cap_w));
  HIP_TRY(c->front_spill.ensure(dc::front_spill_words()));
  const bool dedup = (knobs().front_dedup >> ((depth == 7 ? 0 : 2) + (n_shards > 1 ? 1 : 0))) & 1;
  dc::FrontDedup dd{};
  if (dedup) {
    constexpr u32 kSlots = 2 * (u32)dc::kMoveWordNodesMax;  // at most cap_b owners: half full
    static_assert(kSlots <= 1u << 21, "a record's slot word keeps the slot in 21 bits");
    HIP_TRY(c->fd_key.ensure(kSlots));
    HIP_TRY(c->fd_owner.ensure(kSlots));
    HIP_TRY(c->fd_total.ensure((size_t)cap_b + 256));  // (+ a group's span: k_count3c's flush)
    HIP_TRY(c->fd_rec_slot.ensure(cap_b));
    HIP_TRY(c->fd_rec_flags.ensure(cap_b));
    HIP_TRY(c->fd_rec_board.ensure(cap_b));
    HIP_TRY(c->fd_state.ensure(1));
    if (c->fd_clean_key != c->fd_key.p || c->fd_clean_state != c->fd_state.p) {
      HIP_TRY(hipMemsetAsync(c->fd_key.p, 0, (size_t)kSlots * sizeof(u64), c->stream));
      HIP_TRY(hipMemsetAsync(c->fd_state.p, 0, sizeof(dc::FrontDedupState), c->stream));
    }
    // not clean again until the sequence below is enqueued to its end
    c->fd_clean_key = nullptr;
    c->fd_clean_state = nullptr;
    dd = dc::FrontDedup{c->fd_key.p,      c->fd_owner.p,     c->fd_total.p, c->fd_rec_slot.p, c->fd_rec_flags.p,
                        c->fd_rec_board.p, c->fd_state.p,     c->front_hash_mask, kSlots - 1, cap_b};
  }
  if (dedup) {
    HIP_TRY(c->fd_desc.ensure(1));
    if (c->fd_desc_at != c->fd_desc.p || std::memcmp(&c->fd_desc_host, &dd, sizeof(dd)) != 0) {
      c->fd_desc_host = dd;  // (the copy's source outlives the call)
      HIP_TRY(hipMemcpyAsync(c->fd_desc.p, &c->fd_desc_host, sizeof(dd), hipMemcpyHostToDevice, c->stream));
      c->fd_desc_at = c->fd_desc.p;
    }
  }
  c->last_front_dedup = dedup;
  if (stage_root) {
    e = write_root_host(c, pos, 1);
    if (e == DC_SUCCESS) e = upload_roots(c, 1, false);  // (REF: no meta)
    if (e != DC_SUCCESS) return e;
  }
  dc::Range* rng = c->rng.p + 8;  // [8] the grandparents, [9] the move words
  HIP_TRY(c->timed("front", 0, [&] {
    return dc::launch_front(c->stream, pos->stm, depth, c->root.p, shard, n_shards, c->nodes[0].p, c->tags[0].p,
                            cap_b, c->move_words.p, cap_w, c->res.p, rng, fst, c->front_spill.p,
                            dedup ? c->fd_desc.p : nullptr);
  }));
  c->last_final = "count2";
  const int stm_g = pos->stm ^ (int)((depth - 3) & 1);  // the grandparents are ply depth - 3
  HIP_TRY(c->timed("count2", 0, [&] {
    return dc::launch_count3c(c->stream, stm_g, c->nodes[0].p, c->tags[0].p, rng, rng + 1, c->move_words.p,
                              c->res.p, nullptr, fst, dedup ? dd.gp_total : nullptr);
  }));
  if (dedup) {
    HIP_TRY(c->timed("fold", 0, [&] { return dc::launch_front_fold(c->stream, dd, c->nodes[0].p, rng, c->res.p); }));
    c->fd_clean_key = c->fd_key.p;
    c->fd_clean_state = c->fd_state.p;
  }
  return DC_SUCCESS;
}

// A deduplicating sequence that failed part-way leaves the table unclean
// (fd_clean_*): the next front_enqueue clears it in full, but a captured graph
// would replay without that clear and decline run after run, so the captured
// graphs are dropped with it.
static int front_enqueue(dc_ctx* c, const PerftReq& q, bool stage_root) {
  const int e = front_enqueue_seq(c, q, stage_root);
  if (e != DC_SUCCESS && c->fd_key.p && c->fd_clean_key != c->fd_key.p) {
    for (GraphExecHandle* ge : {&c->pgraph, &c->rgraph, &c->rgraph_batch}) ge->reset();
  }
  return e;
}

// The frontier of one run while it is built: k_expand_top to level T, then one
// level per count_and_scan + write_next, with this rank's shard taken at level
// S.  dc_perft and dc_perft_stats drive it; what each level's capacity is, and
// which final stage takes over where, is theirs to decide.
struct LevelChain {
  dc_ctx* c;
  const PerftReq& q;
  bool exact;        // level sizes are read back (size_level / size_next) instead of bounded,
  bool* host_sync;   // which sets this: the sequence then depends on data (never captured)
  bool sharded;      // a shard of level S is taken
  u32 S, T;
  bool top_words;    // level T is still k_expand_top's move words: the first count_and_scan makes it
  bool shard_words;  // ... and makes only this rank's strided shard of it (S == T)
  dc::TopScratch ts{};
  u32 L = 0;   // the current level,
  u64 nb = 0;  // the bound of its node count,
  int buf = 0;  // and which of the ping-pong level buffers holds it
  // Level L's counts and chunk sums live in buffer pair cb; the k_level_write
  // that makes level L + 1 can count it into the other pair (counted: no
  // k_level_count launch for it).
  int cb = 0;
  bool counted = false;

  bool fide() const { return q.fide(); }
  int stm() const { return q.pos->stm ^ (int)(L & 1); }  // the side to move at level L
  uint16_t* meta(int b) const { return fide() ? c->meta[b].p : nullptr; }
  DBuf<u32>& counts(int k) const { return k ? c->counts2 : c->counts; }
  DBuf<u64>& sums(int k) const { return k ? c->chunk_sum2 : c->chunk_sum; }

  // The buffers of the top (allocated before anything is enqueued) and the root
  // upload from pinned memory (stage_root = false: the caller staged it).
  int begin(u64 cap_T, bool stage_root, bool upload_meta) {
    int e = perft_ensure_common(c);
    if (e != DC_SUCCESS) return e;
    HIP_TRY(c->top_nodes.ensure(kTopCap[1] + kTopCap[2]));
    HIP_TRY(c->top_tags.ensure(kTopCap[1] + kTopCap[2]));
    if (fide()) HIP_TRY(c->top_meta.ensure(kTopCap[1] + kTopCap[2]));
    e = ensure_level(c, 0, cap_T, fide());
    if (e != DC_SUCCESS) return e;
    if (top_words) HIP_TRY(c->top_words.ensure(cap_T));
    for (int k = 0; k < 2; ++k) {
      const u64 off = k ? kTopCap[1] : 0;
      ts.nodes[k] = c->top_nodes.p + off;
      ts.tags[k] = c->top_tags.p + off;
      ts.meta[k] = fide() ? c->top_meta.p + off : nullptr;
      ts.cap[k] = kTopCap[k + 1];
    }
    L = T;
    nb = cap_T;
    if (!stage_root) return DC_SUCCESS;
    e = write_root_host(c, q.pos, q.n_pos);
    return e == DC_SUCCESS ? upload_roots(c, q.n_pos, upload_meta) : e;
  }

  // Level T (the result block is cleared by k_expand_top itself: its first stores).
  int expand_top() {
    HIP_TRY(c->timed("expand_top", 0, [&] {
      return dc::launch_expand_top(c->stream, q.rules, c->root.p, c->root_meta.p, q.pos->stm, T, ts, c->nodes[0].p,
                                   meta(0), c->tags[0].p, nb, c->res.p, c->rng.p + T,
                                   top_words ? c->top_words.p : nullptr, q.n_pos);
    }));
    return L == S ? take_shard() : DC_SUCCESS;
  }

  // This rank's shard of level L (= S).
  int take_shard() {
    if (!sharded) return DC_SUCCESS;
    if (shard_words) {  // the words stay whole: only the level's Range becomes the shard's
      HIP_TRY(dc::launch_shard_range(c->stream, c->rng.p + L, q.shard, q.n_shards));
      return DC_SUCCESS;
    }
    int e = ensure_level(c, buf ^ 1, nb, fide());
    if (e != DC_SUCCESS) return e;
    HIP_TRY(dc::launch_gather_shard(c->stream, c->nodes[buf].p, meta(buf), c->tags[buf].p, c->rng.p + L, q.shard,
                                    q.n_shards, c->nodes[buf ^ 1].p, meta(buf ^ 1), c->tags[buf ^ 1].p));
    buf ^= 1;
    return DC_SUCCESS;
  }

  // Exact mode: the real size of level L (of level L + 1, once scanned) instead of its bound.
  int size_level() { return exact ? read_size(L, &nb) : DC_SUCCESS; }
  int size_next(u64* n) { return exact ? read_size(L + 1, n) : DC_SUCCESS; }
  int read_size(u32 level, u64* n) {
    *host_sync = true;
    return read_range(c, (int)level, n);
  }

  // Level L's counts + chunk sums, then the chunk scan into Range L + 1 (capacity
  // cap; guard: see launch_chunk_scan).  count_next: level L + 1 will be counted
  // by the write that makes it (its chunk sums are cleared here).
  int count_and_scan(u64 cap, u64 guard, bool count_next) {
    const u64 nch = std::max<u64>(dc::chunks_for(nb), 1);
    HIP_TRY(counts(cb).ensure(std::max<u64>(nb, 1)));
    HIP_TRY(sums(cb).ensure(nch));
    HIP_TRY(c->chunk_base.ensure(nch));
    const u64 nch_next = std::max<u64>(dc::chunks_for(std::min<u64>(cap, 0xFFFFFFFFull)), 1);
    if (count_next) {
      HIP_TRY(counts(cb ^ 1).ensure(std::max<u64>(std::min<u64>(cap, 0xFFFFFFFFull), 1)));
      HIP_TRY(sums(cb ^ 1).ensure(nch_next));
    }
    if (top_words) {  // level T, left as move words by k_expand_top
      top_words = false;
      HIP_TRY(c->timed("expand_count", 0, [&] {
        return dc::launch_make_count(c->stream, q.rules, stm() ^ 1, ts.nodes[T - 2], ts.meta[T - 2], ts.tags[T - 2],
                                     c->top_words.p, c->rng.p + L, nb, c->nodes[buf].p, meta(buf), c->tags[buf].p,
                                     counts(cb).p, sums(cb).p, shard_words ? q.shard : 0u,
                                     shard_words ? q.n_shards : 1u);
      }));
    } else if (!counted) {
      HIP_TRY(c->timed("expand_count", 0, [&] {
        return dc::launch_level_count(c->stream, q.rules, stm(), c->nodes[buf].p, meta(buf), c->rng.p + L, nb,
                                      counts(cb).p, sums(cb).p);
      }));
    }
    HIP_TRY(c->timed("scan", 0, [&] {
      return dc::launch_chunk_scan(c->stream, sums(cb).p, c->rng.p + L, c->chunk_base.p, c->rng.p + L + 1, cap,
                                   c->res.p, 0, guard, count_next ? sums(cb ^ 1).p : nullptr, nch_next);
    }));
    return DC_SUCCESS;
  }

  // Level L + 1 (capacity cap_next) written from level L, which it replaces as
  // the current one; the shard is taken if it is level S.
  int write_next(u64 cap_next, bool count_next) {
    int e = ensure_level(c, buf ^ 1, cap_next, fide());
    if (e != DC_SUCCESS) return e;
    HIP_TRY(c->timed("expand_write", 0, [&] {
      return dc::launch_level_write(c->stream, q.rules, stm(), c->nodes[buf].p, meta(buf), c->tags[buf].p,
                                    c->rng.p + L, nb, counts(cb).p, c->chunk_base.p, c->nodes[buf ^ 1].p,
                                    meta(buf ^ 1), c->tags[buf ^ 1].p, cap_next,
                                    count_next ? counts(cb ^ 1).p : nullptr, count_next ? sums(cb ^ 1).p : nullptr);
    }));
    buf ^= 1;
    counted = count_next;
    if (count_next) cb ^= 1;
    ++L;
    nb = cap_next;
    return L == S ? take_shard() : DC_SUCCESS;
  }
};

// Enqueues one perft on the context stream up to (not including) the result
// copy.  *host_sync is set when a level size had to be read back on the host
// (exact mode or a level beyond the speculative budget): such a sequence
// depends on data and is never captured as a graph.
int perft_enqueue(dc_ctx* c, const PerftReq& q, bool exact, bool front, bool stage_root, bool* host_sync) {
  if (front && !exact) return front_enqueue(c, q, stage_root);
  const PerftShape sh = perft_shape(q, exact);
  if (sh.Ldfs > 3) return DC_EUNSUPPORTED;
  u32 F = sh.F, Ldfs = sh.Ldfs;  // (exact mode may move both to K4 below)
  const bool wide = sh.wide, sliced = sh.sliced, fused3 = sh.fused3;
  LevelChain ch{c, q, exact, host_sync, q.sharded(), sh.S, sh.T, sh.top_words, sh.shard_words};
  int e = ch.begin(sh.cap_T, stage_root, q.fide());
  if (e != DC_SUCCESS) return e;
  // Capacity of level L + 1 (and the node guard of level L) in speculative
  // mode: the move-word level of the fused final stage, else a board level.
  auto spec_cap = [&](u32 lvl, u64 n_lvl, u64* guard) -> u64 {
    if (fused3 && wide && lvl + 1 == F) {  // 64-bit words: no grandparent limit
      *guard = 0;
      return std::min<u64>(n_lvl * kBranchBound, wide_words_max());
    }
    if (fused3 && lvl + 1 == F) {
      *guard = dc::kMoveWordNodesMax;
      return std::min<u64>(std::min<u64>(n_lvl, dc::kMoveWordNodesMax) * kBranchBound, 0xFFFFFFFFull);
    }
    *guard = 0;
    if (sliced && lvl + 2 == F)  // the sliced stage's grandparents (a lowered budget: tests)
      return std::min(n_lvl * kBranchBound, std::min(kSpecBudget, wide_level_bytes()) / kNodeBytes);
    return std::min(n_lvl * kBranchBound, kSpecBudget / kNodeBytes);
  };
  // the fused final stage over level L's children as move words (u64 when wide)
  auto fused_stage = [&](auto* words, const Board* nodes, const uint16_t* tags, const dc::Range* rng, u64 n_bound,
                         const u32* counts, const u64* chunk_base, u64 cap_w, u32* counter) -> int {
    const int stm = ch.stm();
    HIP_TRY(c->timed("level_moves", 0, [&] {
      return dc::launch_level_moves(c->stream, stm, nodes, rng, n_bound, counts, chunk_base, words, cap_w);
    }));
    c->last_final = "count2";
    HIP_TRY(c->timed("count2", 0, [&] {
      return dc::launch_count3c(c->stream, stm, nodes, tags, rng, rng + 1, words, c->res.p, counter);
    }));
    return DC_SUCCESS;
  };
  e = ch.expand_top();
  if (e != DC_SUCCESS) return e;
  while (ch.L < F) {
    const u32 L = ch.L;
    e = ch.size_level();
    if (e != DC_SUCCESS) return e;
    const Board* nodes = c->nodes[ch.buf].p;
    const uint16_t* tags = c->tags[ch.buf].p;
    if (fused3 && sliced && L + 1 == F) {
      // words of the whole level are never stored: per slice of grandparents,
      // k_level_moves writes that slice's words and k_count3c counts them
      e = ch.count_and_scan(~0ull, 0, false);
      if (e != DC_SUCCESS) return e;
      const u64 cap_w = std::min<u64>(kSliceNodes * 256, kWideWordsMax);
      HIP_TRY(c->move_words64.ensure(cap_w));
      HIP_TRY(c->slice_rng.ensure(2));
      HIP_TRY(c->slice_ctr.ensure(1));
      const u64 n_slices = std::max<u64>((ch.nb + kSliceNodes - 1) / kSliceNodes, 1);
      c->last_final = "count2";
      for (u64 k = 0; k < n_slices; ++k) {
        const u64 s0 = k * kSliceNodes;
        HIP_TRY(dc::launch_wide_slice(c->stream, c->rng.p + L, c->chunk_base.p, c->rng.p + L + 1, s0, kSliceNodes,
                                      c->slice_rng.p, c->slice_ctr.p, c->res.p, cap_w));
        e = fused_stage(c->move_words64.p, nodes + s0, tags + s0, c->slice_rng.p, kSliceNodes,
                        ch.counts(ch.cb).p + s0, c->chunk_base.p + dc::chunks_for(s0), cap_w, c->slice_ctr.p);
        if (e != DC_SUCCESS) return e;
      }
      return DC_SUCCESS;
    }
    if (fused3 && L + 1 == F && (!exact || wide || ch.nb <= dc::kMoveWordNodesMax)) {
      // one u32 move word per child (u64 when wide); in speculative mode a
      // grandparent level past kMoveWordNodesMax (a word level past
      // kWideWordsMax) is flagged on the device (exact rerun)
      u64 guard = 0;
      u64 cap_f = spec_cap(L, ch.nb, &guard);
      e = ch.count_and_scan(exact ? ~0ull : cap_f, exact ? 0 : guard, false);
      if (e == DC_SUCCESS) e = ch.size_next(&cap_f);
      if (e != DC_SUCCESS) return e;
      if (exact && wide && cap_f > wide_words_max()) {
        // too many words for the fused stage: K4 from this level (ply 5)
        Ldfs = F - L;
        F = L;
        break;
      }
      if (exact && cap_f > 0xFFFFFFFFull) return DC_EUNSUPPORTED;
      if (wide) {
        HIP_TRY(c->move_words64.ensure(std::max<u64>(cap_f, 1)));
        return fused_stage(c->move_words64.p, nodes, tags, c->rng.p + L, ch.nb, ch.counts(ch.cb).p, c->chunk_base.p,
                           cap_f, nullptr);
      }
      HIP_TRY(c->move_words.ensure(std::max<u64>(cap_f, 1)));
      return fused_stage(c->move_words.p, nodes, tags, c->rng.p + L, ch.nb, ch.counts(ch.cb).p, c->chunk_base.p, cap_f,
                         nullptr);
    }
    // Speculative mode never reads a level size back: the next level gets
    // min(64 x bound, kSpecBudget) of capacity, a level past it is dropped and
    // flagged (k_chunk_scan) and the run redone in exact mode.  The level
    // kernels use resident grids over device Ranges, so a loose bound costs
    // memory, not launches.  (Reading the ply-4 size back cost perft(7) one
    // host sync mid-run and kept it out of the graph.)
    u64 guard_unused = 0;
    u64 cap_next = exact ? ch.nb * kBranchBound : spec_cap(L, ch.nb, &guard_unused);
    // the write counts level L + 1 when that level is counted next (not the
    // final stage's level, not a level first cut to this rank's shard)
    // (speculative mode only: exact mode sizes the next level after the scan)
    const bool count_next = !exact && L + 1 < F && !(ch.sharded && L + 1 == ch.S);
    e = ch.count_and_scan(exact ? ~0ull : cap_next, 0, count_next);
    if (e == DC_SUCCESS) e = ch.size_next(&cap_next);
    if (e != DC_SUCCESS) return e;
    if (exact && sliced && L + 2 == F && cap_next * kNodeBytes > wide_level_bytes()) {
      // the sliced stage's grandparent level would not fit: K4 from this level
      Ldfs = F - L;
      F = L;
      break;
    }
    if (exact && cap_next > 0xFFFFFFFFull) return DC_EUNSUPPORTED;
    e = ch.write_next(cap_next, count_next);
    if (e != DC_SUCCESS) return e;
  }
  const int buf = ch.buf;
  c->last_final = Ldfs > 0 ? "dfs" : sh.final_plies == 2 ? "count2" : "count1";
  if (Ldfs > 0) {
    const u64 lanes = dc::dfs_lanes();
    if (Ldfs > 1) HIP_TRY(c->dfs_stack.ensure((size_t)(Ldfs - 1) * 7 * lanes));
    HIP_TRY(c->timed("dfs", 0, [&] {
      return dc::launch_perft_dfs(c->stream, ch.stm() ^ (int)(Ldfs & 1), Ldfs, c->nodes[buf].p, c->tags[buf].p,
                                  c->rng.p + ch.L, c->res.p, Ldfs > 1 ? c->dfs_stack.p : nullptr, lanes);
    }));
  } else if (q.depth >= 2) {
    HIP_TRY(c->timed(sh.final_plies == 2 ? "count2" : "count1", 0, [&] {
      return dc::launch_final(c->stream, q.rules, ch.stm(), sh.final_plies, c->nodes[buf].p, ch.meta(buf),
                              c->tags[buf].p, c->rng.p + ch.L, ch.nb, c->res.p->divide);
    }));
  }
  return DC_SUCCESS;
}

// What a captured sequence depends on, with the allocation epoch as of now.
static dc_ctx::PerftKey perft_key(const PerftReq& q, bool front) {
  return dc_ctx::PerftKey{q.rules, q.depth, q.split_depth, q.shard, q.n_shards, (u32)q.pos->stm,
                          (u32)perft_k4_forced(), q.n_pos, g_alloc_epoch.load(), wide_words_max(), wide_level_bytes(),
                          front};
}

// Ends the capture on the context stream and instantiates the graph into *out
// (best effort: *out is nullptr unless everything, the enqueueing included,
// went well and no buffer moved since the key's epoch).
static bool end_capture(dc_ctx* c, uint64_t key_epoch, bool ok_so_far, hipGraphExec_t* out) {
  hipGraph_t g = nullptr;
  const hipError_t ee = hipStreamEndCapture(c->stream, &g);
  const bool ok = ok_so_far && ee == hipSuccess && g && key_epoch == g_alloc_epoch.load() &&
                  hipGraphInstantiate(out, g, nullptr, nullptr, 0) == hipSuccess;
  if (!ok) *out = nullptr;
  if (g) (void)hipGraphDestroy(g);
  (void)hipGetLastError();
  return ok;
}

// One perft.  A repeated configuration (same rules, depth, shard, side to move
// and buffers) replays the launch sequence captured from its previous run as a
// hipGraph: the 12 stream operations of a perft(7) go to the GPU as one launch,
// which removes the per-kernel launch gaps.  The root position
// is read from the pinned staging block when the graph runs.
int perft_run(dc_ctx* c, const PerftReq& q, bool exact, bool front, dc::PerftResult* out) {
  const bool graphable = !exact && !c->profiling;
  front = front && !exact;
  const dc_ctx::PerftKey key = perft_key(q, front);
  if (graphable && c->pgraph && c->pkey == key) {
    int e = write_root_host(c, q.pos, q.n_pos);
    if (e != DC_SUCCESS) return e;
    HIP_TRY(hipGraphLaunch(c->pgraph, c->stream));
    e = sync_ctx(c);
    if (e != DC_SUCCESS) return e;
    *out = *c->res_host;
    return DC_SUCCESS;
  }
  bool host_sync = false;
  int e = perft_enqueue(c, q, exact, front, true, &host_sync);
  if (e != DC_SUCCESS) return e;
  HIP_TRY(hipMemcpyAsync(c->res_host, c->res.p, sizeof(dc::PerftResult), hipMemcpyDeviceToHost, c->stream));
  e = sync_ctx(c);
  if (e != DC_SUCCESS) return e;
  *out = *c->res_host;
  if (!graphable || host_sync || out->overflow) return DC_SUCCESS;
  // capture the same sequence for the next call (best effort: any failure
  // leaves the plain path in place)
  c->pgraph.reset();
  if (hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
    (void)hipGetLastError();
    return DC_SUCCESS;
  }
  bool hs = false;
  int ce = perft_enqueue(c, q, false, front, true, &hs);
  if (ce == DC_SUCCESS &&
      hipMemcpyAsync(c->res_host, c->res.p, sizeof(dc::PerftResult), hipMemcpyDeviceToHost, c->stream) != hipSuccess)
    ce = DC_EHIP;
  if (end_capture(c, key.epoch, ce == DC_SUCCESS && !hs, &c->pgraph.h)) c->pkey = key;
  return DC_SUCCESS;
}

// The request's own fields as the C ABI bounds them (every entry point checks its pointers besides).
static int check_request(const PerftReq& q) {
  if (!q.pos || q.rules > DC_RULES_FIDE || q.n_shards == 0 || q.shard >= q.n_shards || q.pos->stm > 1) return DC_EINVAL;
  return q.depth > 12 ? DC_EUNSUPPORTED : DC_SUCCESS;
}

// root_parent (a batch): which root position each root move belongs to, or null
int perft_impl(dc_ctx* c, const PerftReq& q, uint64_t* divide, uint16_t* root_moves, uint32_t* n_root,
               uint64_t* total, uint8_t* root_parent) {
  if (!total) return DC_EINVAL;
  if (int bad = check_request(q)) return bad;
  const uint32_t depth = q.depth, shard = q.shard;
  *total = 0;
  if (n_root) *n_root = 0;
  if (depth == 0) {
    *total = (shard == 0) ? 1 : 0;
    return DC_SUCCESS;
  }
  dc::PerftResult r;
  // the one-launch front end where eligible; a position it declines (a top
  // past its LDS bounds, a level past its capacity) takes the legacy chain,
  // and speculative capacities that overflow there the exact rerun
  bool front = front_eligible(q);
  int e = perft_run(c, q, false, front, &r);
  if (e == DC_SUCCESS && front && r.overflow && r.front_declined) {
    front = false;
    e = perft_run(c, q, false, false, &r);
  }
  c->last_front = front;
  c->last_exact = e == DC_SUCCESS && r.overflow;
  if (c->last_exact) e = perft_run(c, q, true, false, &r);
  if (e != DC_SUCCESS) return e;
  if (r.overflow) return DC_EUNSUPPORTED;  // more than 256 root moves, or a level beyond 2^32 nodes
  const u32 nr = r.n_root;
  if (n_root) *n_root = nr;
  if (root_moves) std::copy(r.root_moves, r.root_moves + nr, root_moves);
  if (root_parent) std::copy(r.root_parent, r.root_parent + nr, root_parent);
  u64 t = 0;
  for (u32 i = 0; i < nr; ++i) {
    const u64 v = depth == 1 ? (shard == 0 ? 1 : 0) : r.divide[i];
    t += v;
    if (divide) divide[i] = v;
  }
  *total = t;
  if (c->profiling && depth >= 2) {
    auto it = c->stats.find(c->last_final);  // the final stage that ran
    if (it != c->stats.end()) it->second.units += t;
  }
  return DC_SUCCESS;
}

// ========================================================= perft statistics
// dc_perft_stats: the frontier at ply depth - 1 is built as boards, meta and
// tags by the LevelChain alone, its move-word top and counting write switched
// off (k_expand_top, then k_level_count, k_chunk_scan and k_level_write per
// level, the shard cut at split_depth included; no k_front, no move-word
// level, no k_count3c), and k_leaf_stats classifies every move of every
// frontier node into the counter block c->pstats.  Speculative capacities
// (within c->stats_level_cap besides) and the exact mode are perft_enqueue's.
constexpr size_t kStatsWords = 256 * (size_t)dc::kPsCount;

int stats_enqueue(dc_ctx* c, const PerftReq& q, bool exact) {
  const bool fide = q.fide();
  const u32 F = q.depth - 1;            // the frontier's ply; 0: the root itself (depth 1)
  const u32 Fb = std::max<u32>(F, 1);   // the deepest ply built (ply 1 gives the root moves)
  const u32 S = shard_level(q.split_depth, Fb);
  const u32 T = top_plies(fide, exact, Fb, q.sharded(), S);
  // (the test knob bounds the speculative top ply as it does the levels below)
  const u64 cap_T = exact ? kTopCap[T] : std::min(kTopCap[T], c->stats_level_cap);
  HIP_TRY(c->pstats.ensure(kStatsWords));
  if (!c->pstats_host) HIP_TRY(c->pstats_host.alloc(hipHostMallocDefault, kStatsWords * sizeof(u64)));
  bool host_sync = false;  // (nothing here is captured)
  // boards at every level, every n-th node as the shard; at depth 1 nothing is
  // cut (shard 0 holds the root's moves, as dc_perft_shard's depth 1)
  LevelChain ch{c, q, exact, &host_sync, q.sharded() && F > 0, S, T, false, false};
  // (the meta goes up under REF too: the device root then always equals the
  // staged one, which is what root_staged lets a later captured run assume)
  int e = ch.begin(cap_T, true, true);
  if (e != DC_SUCCESS) return e;
  HIP_TRY(hipMemsetAsync(c->pstats.p, 0, kStatsWords * sizeof(u64), c->stream));
  e = ch.expand_top();
  if (e != DC_SUCCESS) return e;
  if (F == 0) {
    if (q.shard != 0) return DC_SUCCESS;
    HIP_TRY(c->timed("leaf_stats", 0, [&] {
      return dc::launch_leaf_stats(c->stream, q.rules, q.pos->stm, c->root.p, fide ? c->root_meta.p : nullptr, nullptr,
                                   nullptr, 1, c->res.p, 1, c->pstats.p);
    }));
    return DC_SUCCESS;
  }
  while (ch.L < F) {
    e = ch.size_level();
    if (e != DC_SUCCESS) return e;
    u64 cap_next = std::min(std::min(ch.nb * kBranchBound, kSpecBudget / kNodeBytes), c->stats_level_cap);
    e = ch.count_and_scan(exact ? ~0ull : cap_next, 0, false);
    if (e == DC_SUCCESS) e = ch.size_next(&cap_next);
    if (e != DC_SUCCESS) return e;
    if (exact && cap_next > 0xFFFFFFFFull) return DC_EUNSUPPORTED;
    e = ch.write_next(cap_next, false);
    if (e != DC_SUCCESS) return e;
  }
  HIP_TRY(c->timed("leaf_stats", 0, [&] {
    return dc::launch_leaf_stats(c->stream, q.rules, ch.stm(), c->nodes[ch.buf].p, ch.meta(ch.buf), c->tags[ch.buf].p,
                                 c->rng.p + F, ch.nb, c->res.p, 0, c->pstats.p);
  }));
  return DC_SUCCESS;
}


int stats_run(dc_ctx* c, const PerftReq& q, bool exact, dc::PerftResult* out) {
  int e = stats_enqueue(c, q, exact);
  if (e != DC_SUCCESS) return e;
  HIP_TRY(hipMemcpyAsync(c->res_host, c->res.p, sizeof(dc::PerftResult), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(c->pstats_host, c->pstats.p, kStatsWords * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  e = sync_ctx(c);
  if (e != DC_SUCCESS) return e;
  *out = *c->res_host;
  return DC_SUCCESS;
}

int stats_impl(dc_ctx* c, const PerftReq& q, uint64_t* totals, uint64_t* rows, uint16_t* root_moves,
               uint32_t* n_root) {
  if (!totals) return DC_EINVAL;
  if (int bad = check_request(q)) return bad;
  std::fill(totals, totals + DC_PS_COUNT, 0);
  if (n_root) *n_root = 0;
  if (q.depth == 0) {
    totals[DC_PS_NODES] = (q.shard == 0) ? 1 : 0;
    return DC_SUCCESS;
  }
  dc::PerftResult r;
  int e = stats_run(c, q, false, &r);
  c->last_stats_exact = e == DC_SUCCESS && r.overflow;
  if (c->last_stats_exact) e = stats_run(c, q, true, &r);
  if (e != DC_SUCCESS) return e;
  if (r.overflow) return DC_EUNSUPPORTED;  // more than 256 root moves, or a level beyond 2^32 nodes
  const u32 nr = r.n_root;
  if (n_root) *n_root = nr;
  if (root_moves) std::copy(r.root_moves, r.root_moves + nr, root_moves);
  const u64* st = c->pstats_host;
  for (u32 i = 0; i < nr; ++i)
    for (u32 k = 0; k < DC_PS_COUNT; ++k) totals[k] += st[(size_t)DC_PS_COUNT * i + k];
  if (rows) std::copy(st, st + (size_t)DC_PS_COUNT * nr, rows);
  if (c->profiling) {
    auto it = c->stats.find("leaf_stats");
    if (it != c->stats.end()) it->second.units += totals[DC_PS_NODES];
  }
  return DC_SUCCESS;
}

}  // namespace

extern "C" {

// Test hook (not in the header): the most nodes a speculative level of
// dc_perft_stats may hold (0: unlimited again), so a test can send a small
// tree through the exact rerun.
extern "C" __attribute__((visibility("default"))) int dc_test_perft_stats_level_cap(dc_ctx* c, uint64_t cap) {
  if (!c) return DC_EINVAL;
  c->stats_level_cap = cap ? cap : ~0ull;
  return DC_SUCCESS;
}

// Test hook (not in the header): 1 when the context's last dc_perft_stats took
// the exact rerun, 0 when its speculative capacities held.
extern "C" __attribute__((visibility("default"))) int dc_test_perft_stats_last_exact(const dc_ctx* c) {
  return c ? (int)c->last_stats_exact : -1;
}

int dc_perft_stats(dc_ctx* c, uint32_t rules, const dc_pos* pos, uint32_t depth, uint64_t* totals, uint64_t* rows,
                   uint16_t* root_moves, uint32_t* n_root) {
  ENTER_WORK(c);
  return stats_impl(c, PerftReq{rules, pos, 1, depth, 1, 0, 1}, totals, rows, root_moves, n_root);
}

int dc_perft_stats_shard(dc_ctx* c, uint32_t rules, const dc_pos* pos, uint32_t depth, uint32_t split_depth,
                         uint32_t shard, uint32_t n_shards, uint64_t* totals, uint64_t* rows, uint16_t* root_moves,
                         uint32_t* n_root) {
  ENTER_WORK(c);
  return stats_impl(c, PerftReq{rules, pos, 1, depth, split_depth, shard, n_shards}, totals, rows, root_moves, n_root);
}

// Test hook (not in the header): 1 when the context's last perft ran the
// one-launch front end (k_front), 0 when it took the legacy chain.
extern "C" __attribute__((visibility("default"))) int dc_test_perft_last_front(const dc_ctx* c) {
  return c ? (int)c->last_front : -1;
}

// Test hook (not in the header): boards seen, owners and duplicates of the
// context's last k_front run if it deduplicated its grandparents (zeros if not).
extern "C" __attribute__((visibility("default"))) int dc_test_front_dedup_stats(dc_ctx* c, uint64_t out[3]) {
  if (!c || !out) return DC_EINVAL;
  out[0] = out[1] = out[2] = 0;
  if (!c->last_front_dedup || !c->fd_state.p) return DC_SUCCESS;
  if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return DC_EHIP;
  dc::FrontDedupState st;
  if (hipMemcpy(&st, c->fd_state.p, sizeof(st), hipMemcpyDeviceToHost) != hipSuccess) return DC_EHIP;
  for (int i = 0; i < 3; ++i) out[i] = st.stats[i];
  return DC_SUCCESS;
}

// Test hook (not in the header): a mask ANDed into k_front's board hashes (all
// ones by default), so a test can force hash collisions and check that each is
// caught and the run declined.  k_front reads the mask from the FrontDedup
// descriptor in device memory, which is rewritten here once queued work is
// done; captured perft graphs stay valid and see the new mask on their next
// replay (so a test can drive a decline inside a captured front-path graph).
extern "C" __attribute__((visibility("default"))) int dc_test_front_hash_mask(dc_ctx* c, uint64_t mask) {
  if (!c) return DC_EINVAL;
  if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return DC_EHIP;
  c->front_hash_mask = mask;
  if (c->fd_desc.p && c->fd_desc_at == c->fd_desc.p) {  // (else the next front_enqueue uploads it)
    c->fd_desc_host.hash_mask = mask;
    if (hipMemcpy(c->fd_desc.p, &c->fd_desc_host, sizeof(c->fd_desc_host), hipMemcpyHostToDevice) != hipSuccess)
      return DC_EHIP;
  }
  return DC_SUCCESS;
}

int dc_perft(dc_ctx* c, uint32_t rules, const dc_pos* pos, uint32_t depth, uint64_t* divide, uint16_t* root_moves,
             uint32_t* n_root, uint64_t* total) {
  ENTER_WORK(c);
  return perft_impl(c, PerftReq{rules, pos, 1, depth, 1, 0, 1}, divide, root_moves, n_root, total, nullptr);
}

int dc_perft_shard(dc_ctx* c, uint32_t rules, const dc_pos* pos, uint32_t depth, uint32_t split_depth, uint32_t shard,
                   uint32_t n_shards, uint64_t* divide, uint16_t* root_moves, uint32_t* n_root, uint64_t* total) {
  ENTER_WORK(c);
  return perft_impl(c, PerftReq{rules, pos, 1, depth, split_depth, shard, n_shards}, divide, root_moves, n_root, total,
                    nullptr);
}

// n_runs perfts of one position enqueued back to back on the context stream,
// each run's result left on the device (k_copy_result into d_out + 258 i): no
// host round trip between runs.  The first call of a configuration runs it once
// through perft_impl (host sync), which captures the launch sequence; later
// runs replay that hipGraph.  Returns once the runs are enqueued.
// n_runs runs on context c, run i's result at d_out + 258 i.
// Runs per batch graph of dc_perft_repeat_device (see dc_ctx::rgraph_batch).
constexpr u32 kRepeatBatch = 8;

static int repeat_runs(dc_ctx* c, const PerftReq& q, uint32_t n_runs, uint64_t* d_out) {
  if (n_runs == 0) return DC_SUCCESS;
  HIP_TRY(c->rcur.ensure(1));  // before the key: an allocation moves the epoch
  // (a graph captured after a declined front holds the legacy chain: front false)
  dc_ctx::PerftKey key = perft_key(q, front_eligible(q));
  const bool graphable = !c->profiling;
  // capture `runs` runs of the sequence back to back (the result copy is part
  // of the graph: its destination is the cursor)
  auto capture = [&](u32 runs, hipGraphExec_t* out) {
    if (hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) return false;
    bool hs = false;
    int ce = DC_SUCCESS;
    for (u32 r = 0; r < runs && ce == DC_SUCCESS && !hs; ++r) {
      ce = perft_enqueue(c, q, false, key.front, false, &hs);
      if (ce == DC_SUCCESS && dc::launch_copy_result(c->stream, c->res.p, c->rcur.p) != hipSuccess) ce = DC_EHIP;
    }
    return end_capture(c, key.epoch, ce == DC_SUCCESS && !hs, out);
  };
  if (!c->root_host || !(graphable && c->rgraph && c->rkey == key)) {
    // a plain run (host sync) sizes the buffers and stages the root; then the
    // sequence is captured without the root upload and the readback
    uint64_t total = 0;
    int e = perft_impl(c, q, nullptr, nullptr, nullptr, &total, nullptr);
    if (e != DC_SUCCESS) return e;
    if (c->last_exact) {
      // speculative capacities overflow for this configuration: exact runs
      // (one host sync per level), each result still left on the device
      HIP_TRY(dc::launch_set_result_cursor(c->stream, c->rcur.p, reinterpret_cast<u64*>(d_out), 0, 1));
      for (u32 i = 0; i < n_runs; ++i) {
        bool hs = false;
        e = perft_enqueue(c, q, true, false, true, &hs);
        if (e != DC_SUCCESS) return e;
        HIP_TRY(dc::launch_copy_result(c->stream, c->res.p, c->rcur.p));
      }
      return DC_SUCCESS;
    }
    key.epoch = g_alloc_epoch.load();
    key.front = c->last_front;
    if (graphable) {
      c->rgraph.reset();
      c->rgraph_batch.reset();
      if (capture(1, &c->rgraph.h)) {
        c->rkey = key;
        if (n_runs >= kRepeatBatch) (void)capture(kRepeatBatch, &c->rgraph_batch.h);
      }
      (void)hipGetLastError();
    } else {
      c->rgraph_batch.reset();
    }
  }
  const bool use_graph = graphable && c->rgraph && c->rkey == key;
  if (use_graph && !root_staged(c, q.pos, q.n_pos)) {
    // every staging copies root_host to the device root, so the device root
    // holds *pos once queued work is done if root_host does; else restage
    // (write_root_host waits for the runs still queued to read the pinned block)
    int e = write_root_host(c, q.pos, q.n_pos);
    if (e == DC_SUCCESS) e = upload_roots(c, q.n_pos, true);
    if (e != DC_SUCCESS) return e;
  }
  HIP_TRY(dc::launch_set_result_cursor(c->stream, c->rcur.p, reinterpret_cast<u64*>(d_out), 0, 1));
  u32 i = 0;
  if (use_graph && n_runs >= kRepeatBatch && !c->rgraph_batch && c->rgraph) {
    // the key's one-run graph exists but no batch graph yet (an earlier call
    // had fewer runs): capture it now
    (void)capture(kRepeatBatch, &c->rgraph_batch.h);
  }
  if (use_graph && c->rgraph_batch)
    for (; i + kRepeatBatch <= n_runs; i += kRepeatBatch) HIP_TRY(hipGraphLaunch(c->rgraph_batch, c->stream));
  for (; i < n_runs; ++i) {
    if (use_graph) {
      HIP_TRY(hipGraphLaunch(c->rgraph, c->stream));  // perft + result copy
    } else {
      bool host_sync = false;
      int e = perft_enqueue(c, q, false, key.front, true, &host_sync);
      if (e != DC_SUCCESS) return e;
      HIP_TRY(dc::launch_copy_result(c->stream, c->res.p, c->rcur.p));
    }
  }
  return DC_SUCCESS;
}

int dc_perft_repeat_device(dc_ctx* c, uint32_t rules, const dc_pos* pos, uint32_t depth, uint32_t split_depth,
                           uint32_t shard, uint32_t n_shards, uint32_t n_runs, uint64_t* d_out) {
  ENTER_WORK(c);
  if (!pos || (n_runs && !d_out) || rules > DC_RULES_FIDE || n_shards == 0 || shard >= n_shards || pos->stm > 1)
    return DC_EINVAL;
  if (depth < 2 || depth > 12) return DC_EUNSUPPORTED;
  if (n_runs == 0) return DC_SUCCESS;
  // (round 4 measured alternating the runs over a second context, so one
  // run's front end would overlap the other's final stage: 1.03 against
  // 0.53 ms per perft(7) step; not kept)
  return repeat_runs(c, PerftReq{rules, pos, 1, depth, split_depth, shard, n_shards}, n_runs, d_out);
}

// A batch of root positions with the same side to move as one tree: the top
// kernel expands them together, their root moves (at most 256 in all) share
// the divide tags, and every level after it -- the final stage included --
// holds all of them, so the GPU runs one full grid per level instead of one
// small one per position (BASELINE configs[2]: six suite positions at depth 5).
static_assert(DC_PERFT_BATCH_MAX == dc::kMaxPerftRoots, "dchess.h batch bound");
static int batch_args(uint32_t rules, const dc_pos* pos, uint32_t n_pos, uint32_t depth) {
  if (!pos || n_pos == 0 || rules > DC_RULES_FIDE) return DC_EINVAL;
  if (n_pos > dc::kMaxPerftRoots || depth == 0 || depth > 12) return DC_EUNSUPPORTED;
  for (u32 i = 0; i < n_pos; ++i)
    if (pos[i].stm > 1 || pos[i].stm != pos[0].stm) return DC_EINVAL;
  return DC_SUCCESS;
}

int dc_perft_batch(dc_ctx* c, uint32_t rules, const dc_pos* pos, uint32_t n_pos, uint32_t depth, uint64_t* totals,
                   uint64_t* divide, uint16_t* root_moves, uint8_t* root_pos, uint32_t* n_root) {
  ENTER_WORK(c);
  int e = batch_args(rules, pos, n_pos, depth);
  if (e != DC_SUCCESS) return e;
  if (!totals) return DC_EINVAL;
  uint64_t div[256], total = 0;
  uint8_t parent[256];
  uint32_t nr = 0;
  e = perft_impl(c, PerftReq{rules, pos, n_pos, depth, 1, 0, 1}, div, root_moves, &nr, &total, parent);
  if (e != DC_SUCCESS) return e;
  for (u32 i = 0; i < n_pos; ++i) totals[i] = 0;
  // a root move tagged with a position outside the batch can only come from a
  // device fault: an error, never a count folded into some position's total
  for (u32 k = 0; k < nr; ++k)
    if (parent[k] >= n_pos) return DC_EHIP;
  for (u32 k = 0; k < nr; ++k) totals[parent[k]] += div[k];
  if (divide) std::copy(div, div + nr, divide);
  if (root_pos) std::copy(parent, parent + nr, root_pos);
  if (n_root) *n_root = nr;
  return DC_SUCCESS;
}

int dc_perft_batch_repeat_device(dc_ctx* c, uint32_t rules, const dc_pos* pos, uint32_t n_pos, uint32_t depth,
                                 uint32_t split_depth, uint32_t n_runs, uint64_t* d_out) {
  ENTER_WORK(c);
  int e = batch_args(rules, pos, n_pos, depth);
  if (e != DC_SUCCESS) return e;
  if (n_runs && !d_out) return DC_EINVAL;
  if (depth < 2) return DC_EUNSUPPORTED;
  return repeat_runs(c, PerftReq{rules, pos, n_pos, depth, split_depth, 0, 1}, n_runs, d_out);
}

}  // extern "C"
