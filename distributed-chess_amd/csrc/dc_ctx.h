// dc_ctx.h -- the per-device context (stream, grow-only device buffers, pinned
// blocks, HIP-event kernel timing) and the entry helpers shared by the host
// units dc_api*.hip.  Internal: include/dchess.h is the interface.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/dchess.h"
#include "dc_kernels.h"
#include "dc_perft.h"  // the context keeps a FrontDedup by value and stages kMaxPerftRoots roots

using dc::Board;
using dc::DevPos;
using dc::u32;
using dc::u64;

struct LegalIo;  // dc_api_legal.hip
namespace dc {
namespace secp {
struct Ge;  // dc_secp.h (dc_api_txsig.hip)
}
}  // namespace dc

// What the units share that is not inline (hidden: the library's dynamic
// symbols stay the C ABI's).
namespace dcapi __attribute__((visibility("hidden"))) {

// ------------------------------------------------------------------ buffers
// Bumped whenever any device buffer moves: captured perft graphs hold raw
// pointers and are re-captured after a bump.
extern std::atomic<uint64_t> g_alloc_epoch;  // dc_api.hip

// hipFree (and hipHostFree) wait for every stream of the device, a resident
// live-validator wave's included (dc_live_validator): a buffer grown or freed
// while any context's wave runs would block for that wave's lease (up to 60 s).
// LiveHold stops every resident wave of the process first and keeps new ones
// from starting while it is held (those calls take the launched path).
struct LiveHold {  // dc_api_validate.hip
  LiveHold();
  ~LiveHold();
};

// dc_ctx_destroy's part of the live validator: stops the context's wave and
// takes the context off the list LiveHold walks (dc_api_validate.hip).
void live_retire(dc_ctx* c);

// Builds the context's secp256k1 G table on first use (dc_api_txsig.hip).
int ensure_gtab(dc_ctx* c);

}  // namespace dcapi
using dcapi::ensure_gtab;
using dcapi::g_alloc_epoch;
using dcapi::LiveHold;

// The owners below release in their destructors, so dc_ctx lists no buffer by
// hand; none is copyable.
struct NoCopy {
  NoCopy() = default;
  NoCopy(const NoCopy&) = delete;
  NoCopy& operator=(const NoCopy&) = delete;
};

template <class T>
struct DBuf : NoCopy {
  T* p = nullptr;
  size_t cap = 0;
  ~DBuf() { release(); }
  hipError_t ensure(size_t n) {
    if (n <= cap) return hipSuccess;
    LiveHold hold;
    g_alloc_epoch.fetch_add(1);
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    size_t want = std::max<size_t>(n, 64);
    want = want + want / 4;  // grow with headroom
    hipError_t e = hipMalloc(&p, want * sizeof(T));
    if (e != hipSuccess) {
      p = nullptr;
      return e;
    }
    cap = want;
    return hipSuccess;
  }
  void release() {
    if (p) {
      LiveHold hold;
      (void)hipFree(p);
    }
    p = nullptr;
    cap = 0;
  }
};

// One pinned host block (hipHostMalloc / hipHostFree); reads as its pointer.
template <class T>
struct Pinned : NoCopy {
  T* p = nullptr;
  ~Pinned() {
    if (p) {
      LiveHold hold;
      (void)hipHostFree(p);
    }
  }
  hipError_t alloc(unsigned flags = hipHostMallocDefault, size_t bytes = sizeof(T)) {
    return hipHostMalloc((void**)&p, bytes, flags);
  }
  operator T*() const { return p; }
  T* operator->() const { return p; }
};

// One HIP handle (stream, event, graph exec) with its destroy call; reads as the handle.
template <class H, hipError_t (*Destroy)(H)>
struct Handle : NoCopy {
  H h = nullptr;
  ~Handle() { reset(); }
  void reset() {
    if (h) (void)Destroy(h);
    h = nullptr;
  }
  operator H() const { return h; }
};
using StreamHandle = Handle<hipStream_t, hipStreamDestroy>;
using EventHandle = Handle<hipEvent_t, hipEventDestroy>;
using GraphExecHandle = Handle<hipGraphExec_t, hipGraphExecDestroy>;

struct PendingEvent {
  std::string name;
  hipEvent_t a, b;
  u64 units;
};

struct KStat {
  u64 launches = 0;
  double ms = 0;
  u64 units = 0;
};

// Small validate / apply batches (the live consensus call is n = 1: one move
// per block, core/src/consensus/types.rs:10) are staged in one pinned host
// block that the kernel reads and writes in place: no DMA copies, one launch
// and one stream sync per call.  (Three pageable hipMemcpyAsync per call cost
// about 20 of its ~33 us, round 2.)
constexpr uint32_t kHostIoBatch = 4096;
struct HostIo {
  dc_pos pos[kHostIoBatch];
  uint16_t moves[kHostIoBatch];
  uint8_t verdicts[kHostIoBatch];
  uint8_t info[kHostIoBatch];
  uint32_t done;  // one-block launches (n <= 256): the kernel's completion flag (publish_done)
};
constexpr uint32_t kHostFlagBatch = 256;

// Members are destroyed in reverse declaration order, and teardown relies on
// it: the captured graphs (declared last) go before the buffers they point
// into, every event before the stream (~dc_ctx returns the pooled and pending
// ones first), and `stream`, declared first, goes last.  hipFree and
// hipHostFree wait for every stream, so whoever deletes a context holds one
// LiveHold across the delete (dc_ctx_create, dc_ctx_destroy).
struct dc_ctx {
  int device = 0;
  StreamHandle stream;
  bool profiling = false;
  std::vector<hipEvent_t> event_pool;
  std::vector<PendingEvent> pending;
  std::map<std::string, KStat> stats;

  // perft frontier (ping-pong), top-level scratch and per-run control block
  DBuf<Board> nodes[2];
  DBuf<uint16_t> tags[2];
  DBuf<uint16_t> meta[2];  // FIDE castle/ep per node
  DBuf<Board> top_nodes;
  DBuf<uint16_t> top_tags, top_meta;
  DBuf<u32> counts, counts2;        // a level's move counts; counts2: the next level's,
  DBuf<u64> chunk_sum, chunk_sum2;  // made by the k_level_write that writes it
  DBuf<u64> chunk_base;
  DBuf<dc::PerftResult> res;
  DBuf<dc::Range> rng;
  DBuf<u64> dfs_stack;  // K4 frames (dc_perft.hip k_perft_dfs)
  DBuf<Board> root;
  DBuf<uint16_t> root_meta;
  DBuf<dc::ResultCursor> rcur;  // dc_perft_repeat_device: where the next run's result goes
  Pinned<dc::PerftResult> res_host;
  Pinned<u64> replay_host;     // the replay kernel's five counters
  Pinned<u32> plain_host;      // the state hash's names check (k_names_plain's flag)
  EventHandle plain_ev;        // ... recorded after its readback
  Pinned<HostIo> host_io;      // small validate / apply batches, read and written in place
  uint32_t io_seq = 0;         // last completion flag value published into host_io->done / legal_io->done
  Pinned<LegalIo> legal_io;    // dc_legal_moves_batch* (small batches in place; the total)
  // dc_live_validator: the resident wave's mailbox (pinned, coherent), its
  // stream, the requests it has served and its lease (0: off)
  Pinned<dc::LiveBox> live;
  StreamHandle live_stream;
  uint32_t live_seq = 0;
  uint32_t live_lease_us = 0;
  bool live_running = false;
  uint32_t live_timeout_us = 5000000;  // a call the wave neither answers nor leaves in this long is DC_EHIP
  std::mutex live_mu;  // the wave's state: held by live calls and by LiveHold's stop from another thread
  // the last perft_impl needed the exact (host-sized) rerun: its speculative
  // level capacities overflow, so dc_perft_repeat_device must not replay them
  bool last_exact = false;
  // the last perft_impl ran the one-launch front end (k_front); false when it
  // declined the position (the legacy chain ran) or was not eligible
  bool last_front = false;
  const char* last_final = "count2";  // timing name of the last perft's final stage
  struct RootStage {
    Board b[dc::kMaxPerftRoots];
    uint16_t meta[dc::kMaxPerftRoots];
    u32 n;
  };
  Pinned<RootStage> root_host;
  // dc_perft_stats: the counters per root move (256 x DC_PS_COUNT u64, kept out
  // of PerftResult) and their pinned readback block
  DBuf<u64> pstats;
  Pinned<u64> pstats_host;
  // nodes a speculative level of dc_perft_stats may hold (unlimited;
  // dc_test_perft_stats_level_cap lowers it to test the exact rerun)
  u64 stats_level_cap = ~0ull;
  bool last_stats_exact = false;  // the last dc_perft_stats took the exact rerun
  // batch / replay scratch
  DBuf<DevPos> pos;
  DBuf<uint16_t> moves;
  DBuf<uint8_t> verdicts, info;
  // dc_legal_moves_batch*: block sums and bases; the host form's device-side outputs
  DBuf<u32> legal_bsum, legal_bbase, legal_off;
  DBuf<uint8_t> legal_status;
  DBuf<uint16_t> legal_moves;
  DBuf<uint8_t> replay_info;  // dc_replay_info / the state hash's first pass: ply-major [n_plies][n_games] move info
  DBuf<Board> hash_boards;    // the state hash's first pass: every game's final board (round 6)
  DBuf<char> hash_text;    // escaped start history | escaped names of dc_state_hash*
  DBuf<u32> hash_off;      // the names' escaped offsets into hash_text
  DBuf<u32> esc_lens;      // device escaping scratch: per-name escaped lengths,
  DBuf<u64> esc64;         // their scan,
  DBuf<uint8_t> scan_tmp;  // the scan's temporary storage
  DBuf<char> names_raw;    // dc_state_hash (host buffers): the raw names staged
  DBuf<u32> names_raw_off;
  std::string hist_text;   // the escaped start history (host side of the H2D copy)
  DBuf<uint8_t> hashes;
  DBuf<u64> bitmap, digests, stats5;
  // dc_replay_outcome*: the position history of one chunk of games ([slot][word][game],
  // dc_outcome.hip), the block records behind their totals, the host form's outcomes
  DBuf<u64> outcome_hist, outcome_part, outcomes;
  DBuf<uint8_t> san;  // dc_replay_san's host form: ply-major [n_plies][n_games] SAN bytes
  // dc_san_resolve: the host form's tokens and first_bad; either form's five counters
  DBuf<u32> san_tokens, san_first_bad;
  DBuf<u64> san_counts;
  // the *_starts host forms: the per-game clocks and final positions staged (the starts go through pos)
  DBuf<uint16_t> start_clocks;
  DBuf<DevPos> finals;
  // games adjudicated per launch: 1 GiB of history (dc_test_outcome_chunk_games lowers it)
  u32 outcome_chunk_games = 177664;
  // the state hash's replay pre-pass is skipped past this many bytes of its
  // buffers (unlimited; dc_test_hash_prepass_max lowers it to test the fallback)
  u64 hash_prepass_max = ~0ull;
  // the hash kernel keeps move numbers as 32-bit BCD below this bound (at most
  // 10^7; dc_test_hash_bcd_max lowers it to test the division fallback)
  u32 hash_bcd_max = 10000000u;
  DBuf<u32> move_words;  // k_count3c: the final stage's parents as move words below their grandparents
  DBuf<u64> move_words64;  // ... as 64-bit words (REF perft(8): more than 2^20 grandparents)
  DBuf<dc::Range> slice_rng;  // the sliced final stage (REF perft(9)): one slice's node and word Ranges
  DBuf<u32> slice_ctr;        // ... and its group counter
  DBuf<u32> top_words;   // k_expand_top's last ply as move words (k_make_count makes it)
  DBuf<uint8_t> front_st;  // k_front's look-back slots, a dc::FrontState (zeroed once; k_count3c re-zeroes them)
  DBuf<u32> front_spill;   // k_front's spill rows (items past one LDS window)
  uint8_t* front_st_zeroed = nullptr;
  // k_front's transposition dedup (dc::FrontDedup, dc_perft.h): the hash table,
  // each slot's owner index, the owners' totals, the per-board records, the state
  DBuf<u64> fd_key, fd_total;
  DBuf<u32> fd_owner, fd_rec_slot;
  DBuf<uint16_t> fd_rec_flags;
  DBuf<Board> fd_rec_board;
  DBuf<dc::FrontDedupState> fd_state;
  DBuf<dc::FrontDedup> fd_desc;    // the descriptor k_front reads (device copy of fd_desc_host)
  dc::FrontDedup fd_desc_host{};
  dc::FrontDedup* fd_desc_at = nullptr;  // where fd_desc_host was last uploaded
  // the table and state that are known clean (zeroed, and every sequence that
  // used them since was enqueued to its end: its k_front_fold frees what the
  // run claimed); anything else gets a full clear before the next k_front
  u64* fd_clean_key = nullptr;
  dc::FrontDedupState* fd_clean_state = nullptr;
  u64 front_hash_mask = ~0ull;     // ANDed into the board hashes (dc_test_front_hash_mask)
  bool last_front_dedup = false;   // the last k_front enqueued deduplicated
  // transaction-signature check: staged strings / offsets / actions / turns,
  // and the G table (built on first use)
  DBuf<char> tx_text;
  DBuf<u32> tx_off, tx_act;
  DBuf<int8_t> tx_turn;
  DBuf<uint8_t> tx_verdicts;
  DBuf<dc::secp::Ge> gtab;
  bool gtab_ready = false;
  // The last perft launch sequence, captured as a hipGraph (see perft_run).
  // (The graphs hold raw pointers into the buffers above: declared after them.)
  struct PerftKey {
    u32 rules, depth, split, shard, n_shards, stm, k4;
    u32 n_root;  // root positions expanded together (dc_perft_batch; 1 otherwise)
    uint64_t epoch;
    // the capacities a captured graph was sized with (test knobs
    // DCHESS_PERFT_WIDE_MAX / _WIDE_LEVEL_MAX): a changed knob re-captures
    uint64_t wide_words, wide_level;
    bool front;  // the sequence is k_front + k_count3c
    bool operator==(const PerftKey& o) const {
      return rules == o.rules && depth == o.depth && split == o.split && shard == o.shard &&
             n_shards == o.n_shards && stm == o.stm && k4 == o.k4 && n_root == o.n_root && epoch == o.epoch &&
             wide_words == o.wide_words && wide_level == o.wide_level && front == o.front;
    }
  } pkey{};
  GraphExecHandle pgraph;
  // dc_perft_repeat_device's graph: the same sequence without the root upload
  // and the result readback (the root stays on the device between runs)
  GraphExecHandle rgraph;
  // ... and kRepeatBatch runs in one graph: consecutive graph launches leave
  // ~8.6 us between one graph's last kernel and the next graph's first
  // (rocprofv3 kernel trace, round 4), kernels within a graph none
  GraphExecHandle rgraph_batch;
  PerftKey rkey{};

  ~dc_ctx() {
    for (auto& p : pending) {
      (void)hipEventDestroy(p.a);
      (void)hipEventDestroy(p.b);
    }
    for (auto e : event_pool) (void)hipEventDestroy(e);
  }

  hipEvent_t take_event() {
    if (!event_pool.empty()) {
      hipEvent_t e = event_pool.back();
      event_pool.pop_back();
      return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
  }
  // Brackets one launch with events on the context stream when profiling.
  template <class F>
  hipError_t timed(const char* name, u64 units, F&& launch) {
    if (!profiling) return launch();
    PendingEvent pe{name, take_event(), take_event(), units};
    (void)hipEventRecord(pe.a, stream);
    hipError_t e = launch();
    (void)hipEventRecord(pe.b, stream);
    pending.push_back(pe);
    return e;
  }
  // After a stream sync: fold pending events into stats.
  void harvest() {
    for (auto& p : pending) {
      float ms = 0;
      (void)hipEventElapsedTime(&ms, p.a, p.b);
      KStat& s = stats[p.name];
      s.launches++;
      s.ms += ms;
      s.units += p.units;
      event_pool.push_back(p.a);
      event_pool.push_back(p.b);
    }
    pending.clear();
  }
};

#define HIP_TRY(x)                                   \
  do {                                               \
    hipError_t _e = (x);                             \
    if (_e != hipSuccess) return map_hip_error(_e);  \
  } while (0)

static inline int map_hip_error(hipError_t e) {
  static const bool debug = std::getenv("DC_DEBUG") != nullptr;
  if (debug) std::fprintf(stderr, "dchess: HIP error %d (%s)\n", (int)e, hipGetErrorString(e));
  if (e == hipErrorOutOfMemory) return DC_ENOMEM;
  if (e == hipErrorNoDevice || e == hipErrorInvalidDevice) return DC_ENODEV;
  if (e == hipErrorNotSupported) return DC_EUNSUPPORTED;
  return DC_EHIP;
}

static inline int sync_ctx(dc_ctx* c) {
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->harvest();
  return DC_SUCCESS;
}

// Waits for a one-block validate/apply kernel through its host flag
// (publish_done) instead of a stream synchronisation: ~15 us less per n = 1
// call.  A stream that completes or fails without the flag is reported.
static inline uint32_t next_seq(dc_ctx* c) {
  if (++c->io_seq == 0) c->io_seq = 1;  // 0 is the flag's initial value
  return c->io_seq;
}
static inline int wait_host_flag(dc_ctx* c, const uint32_t* flag, uint32_t seq) {
  for (uint32_t k = 1;; ++k) {
    if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) return DC_SUCCESS;
    if ((k & 1023) == 0) {
      const hipError_t q = hipStreamQuery(c->stream);
      if (q == hipSuccess) return __atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq ? DC_SUCCESS : DC_EHIP;
      if (q != hipErrorNotReady) {
        const int e = sync_ctx(c);  // the stream's error
        return e != DC_SUCCESS ? e : DC_EHIP;
      }
    }
  }
}

static inline int enter(dc_ctx* c) {
  if (!c) return DC_EINVAL;
  HIP_TRY(hipSetDevice(c->device));
  return DC_SUCCESS;
}

#define ENTER(c)                      \
  do {                                \
    int _r = enter(c);                \
    if (_r != DC_SUCCESS) return _r;  \
  } while (0)

// Device work other than a live call: every resident live-validator wave of
// the process is stopped first and stays stopped for the call (LiveHold).
// HIP maps a process's streams onto at most GPU_MAX_HW_QUEUES (4) hardware
// queues, so a kernel launched on a stream that shares its queue with a
// resident wave would wait behind that wave for its whole lease (round 5:
// a perft blocked 20 s behind two 20 s leases in the live test module).
#define ENTER_WORK(c) \
  ENTER(c);           \
  LiveHold live_hold_
