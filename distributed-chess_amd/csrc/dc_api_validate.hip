// dc_api_validate.hip -- the live validator (LiveHold included) and
// dc_validate_batch / dc_apply_batch.
#include <chrono>
#include <cstring>
#include <set>

#include "dc_ctx.h"
#include "dc_fide.h"

// Contexts with the live validator on (registered by dc_live_validator,
// removed by dc_ctx_destroy) and the number of LiveHolds alive.  Lock order:
// g_live_mu, then a context's live_mu.
static std::mutex g_live_mu;
static std::set<dc_ctx*> g_live_ctxs;
static std::atomic<int> g_live_hold{0};

// ========================================================= live validator
// dc_live_validator(ctx, lease_us): small validate / apply calls (n <= 64,
// not profiling) go to one resident wave (k_live, dc_moves.hip) through the
// stamped mailbox of dc_kernels.h instead of a kernel launch each.  The wave
// leaves after lease_us without a request (and on dc_live_validator(ctx, 0) or
// dc_ctx_destroy); the next call starts it again.  While it runs, a
// device-wide synchronisation (hipDeviceSynchronize) waits for its lease.
static int live_stop(dc_ctx* c) {
  if (!c->live_running) return DC_SUCCESS;
  __atomic_store_n(&c->live->ctl, 1u, __ATOMIC_RELEASE);
  const hipError_t e = hipStreamSynchronize(c->live_stream);
  __atomic_store_n(&c->live->ctl, 0u, __ATOMIC_RELEASE);
  c->live_running = false;
  return e == hipSuccess ? DC_SUCCESS : DC_EHIP;
}

dcapi::LiveHold::LiveHold() {
  g_live_hold.fetch_add(1);
  std::lock_guard<std::mutex> g(g_live_mu);
  for (dc_ctx* c : g_live_ctxs) {
    std::lock_guard<std::mutex> l(c->live_mu);
    (void)live_stop(c);
  }
}
dcapi::LiveHold::~LiveHold() { g_live_hold.fetch_sub(1); }

void dcapi::live_retire(dc_ctx* c) {
  std::lock_guard<std::mutex> g(g_live_mu);
  std::lock_guard<std::mutex> l(c->live_mu);
  (void)live_stop(c);
  g_live_ctxs.erase(c);
}

static int live_start(dc_ctx* c) {
  __atomic_store_n(&c->live->state, 0u, __ATOMIC_RELEASE);
  __atomic_store_n(&c->live->ctl, 0u, __ATOMIC_RELEASE);
  HIP_TRY(dc::launch_live(c->live_stream, c->live, c->live_seq, (u64)c->live_lease_us * 100));  // 100 MHz clock
  c->live_running = true;
  return DC_SUCCESS;
}

extern "C" {

int dc_live_validator(dc_ctx* c, uint32_t lease_us) {
  ENTER(c);
  if (lease_us > 60u * 1000 * 1000) return DC_EINVAL;  // at most a minute
  if (lease_us && !c->live) {
    HIP_TRY(c->live.alloc(hipHostMallocCoherent));
    std::memset((void*)c->live, 0, sizeof(dc::LiveBox));
  }
  if (lease_us && !c->live_stream) HIP_TRY(hipStreamCreateWithFlags(&c->live_stream.h, hipStreamNonBlocking));
  std::lock_guard<std::mutex> g(g_live_mu);
  std::lock_guard<std::mutex> l(c->live_mu);
  if (lease_us == 0) {
    const int e = live_stop(c);
    c->live_lease_us = 0;
    g_live_ctxs.erase(c);
    return e;
  }
  if (c->live_running && lease_us != c->live_lease_us) {
    const int e = live_stop(c);  // the running wave holds the old lease
    if (e != DC_SUCCESS) return e;
  }
  c->live_lease_us = lease_us;
  g_live_ctxs.insert(c);
  return DC_SUCCESS;
}

// Test hook (not in the header): the live call's no-answer timeout, so a test
// can force the timeout path and check the next call's verdicts.
extern "C" __attribute__((visibility("default"))) int dc_test_live_timeout(dc_ctx* c, uint32_t us) {
  if (!c) return DC_EINVAL;
  std::lock_guard<std::mutex> l(c->live_mu);
  c->live_timeout_us = us;
  return DC_SUCCESS;
}

// live_call's answer when a LiveHold is active: the caller takes the launched path.
constexpr int kLiveDeclined = -1000;

// One request through the mailbox.  pos_out (apply) may alias pos.
// The whole call runs under g_live_mu (then c->live_mu), and whether a hold is
// active is decided under that lock: a LiveHold counts itself before it takes
// g_live_mu, so either this call sees it and declines, or the hold's
// constructor runs after this call and stops the wave it may have started.
// (Round 5 read the hold count and live_running before any lock: a hold that
// stopped the waves in between could be followed by a fresh wave, and the
// hold's hipFree then waited for that wave's lease.)
static int live_call(dc_ctx* c, bool apply, bool fide, const dc_pos* pos, const uint16_t* moves, uint32_t n,
                     uint8_t* verdicts, uint8_t* info, dc_pos* pos_out) {
  std::lock_guard<std::mutex> g(g_live_mu);
  if (g_live_hold.load() != 0) return kLiveDeclined;
  // About to start a wave: the process keeps one resident at a time, since
  // two contexts' live streams may share a hardware queue, where the second
  // wave would wait behind the first for its whole lease.
  if (!c->live_running) {
    for (dc_ctx* o : g_live_ctxs)
      if (o != c) {
        std::lock_guard<std::mutex> l(o->live_mu);
        (void)live_stop(o);
      }
  }
  std::lock_guard<std::mutex> lock(c->live_mu);
  dc::LiveBox* b = c->live;
  if (!c->live_running) {
    const int e = live_start(c);
    if (e != DC_SUCCESS) return e;
  }
  const uint32_t seq = c->live_seq + 1;
  const uint32_t st = dc::live_stamp(seq) << 16;
  if (seq % dc::kLiveClearEvery == 0) std::memset((void*)b->req, 0, sizeof(b->req));
  const uint32_t nw = apply ? dc::kLiveFields * n : n;  // response words read back
  for (uint32_t i = 0; i < nw; ++i) __atomic_store_n(&b->resp[i], 0u, __ATOMIC_RELAXED);
  for (uint32_t e = 0; e < n; ++e) {
    uint16_t h[dc::kLiveFields];
    std::memcpy(h, pos[e].bb, 32);
    h[16] = (uint16_t)(pos[e].stm | (pos[e].castle << 8));
    h[17] = (uint8_t)pos[e].ep;
    h[18] = moves[e];
    for (uint32_t k = 0; k < dc::kLiveFields; ++k) b->req[1 + k * n + e] = st | h[k];
  }
  __atomic_store_n(&b->req[0], st | n | ((uint32_t)apply << 7) | ((uint32_t)fide << 8), __ATOMIC_RELEASE);
  // spin on the response words; a wave that stopped (lease) before taking the
  // request is restarted -- it takes requests only before it publishes state 2
  auto complete = [&]() {
    for (uint32_t i = 0; i < nw; ++i)
      if ((__atomic_load_n(&b->resp[i], __ATOMIC_ACQUIRE) & 0xFFFF0000u) != st) return false;
    return true;
  };
  u64 spins = 0;
  const auto t0 = std::chrono::steady_clock::now();
  while (!complete()) {
    if ((++spins & 255) == 0) {
      if (__atomic_load_n(&b->state, __ATOMIC_ACQUIRE) == 2u) {
        HIP_TRY(hipStreamSynchronize(c->live_stream));
        c->live_running = false;
        if (complete()) break;
        const int e = live_start(c);
        if (e != DC_SUCCESS) return e;
      } else if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(c->live_timeout_us)) {
        (void)live_stop(c);
        // the request may still be in the mailbox, and a wave on its way out
        // may have answered it: clear it and burn its stamp, so the next
        // call's wave looks for seq + 1 and never takes this one for its own
        __atomic_store_n(&b->req[0], 0u, __ATOMIC_RELEASE);
        c->live_seq = seq;
        return DC_EHIP;  // the wave neither answered nor stopped
      }
    }
  }
  c->live_seq = seq;
  for (uint32_t e = 0; e < n; ++e) {
    const uint32_t w = b->resp[e];
    verdicts[e] = (uint8_t)(w & 0xFF);
    if (info) info[e] = (uint8_t)((w >> 8) & 0xFF);
    if (apply) {
      uint16_t h[dc::kLiveFields];
      for (uint32_t k = 1; k < dc::kLiveFields; ++k) h[k] = (uint16_t)b->resp[k * n + e];
      dc_pos q = pos[e];
      std::memcpy(q.bb, h + 1, 32);
      q.stm = (uint8_t)(h[17] & 0xFF);
      q.castle = (uint8_t)(h[17] >> 8);
      q.ep = (int8_t)(uint8_t)h[18];
      pos_out[e] = q;
    }
  }
  return DC_SUCCESS;
}

// (the hold count read here is only a hint; live_call decides under g_live_mu)
static bool live_eligible(const dc_ctx* c, uint32_t n) {
  return c->live_lease_us && n <= dc::kLiveMax && !c->profiling && g_live_hold.load() == 0;
}

// ============================================================== validation
int dc_validate_batch(dc_ctx* c, uint32_t rules, const dc_pos* pos, const uint16_t* moves, uint32_t n,
                      uint8_t* verdicts) {
  ENTER(c);
  if (rules > DC_RULES_FIDE || (n && (!pos || !moves || !verdicts))) return DC_EINVAL;
  if (n == 0) return DC_SUCCESS;
  if (live_eligible(c, n)) {
    const int e = live_call(c, false, rules == DC_RULES_FIDE, pos, moves, n, verdicts, nullptr, nullptr);
    if (e != kLiveDeclined) return e;
  }
  LiveHold live_hold_;  // the launched path (ENTER_WORK)
  if (n <= kHostIoBatch) {  // pinned, read in place by the kernel
    if (!c->host_io) {
      HIP_TRY(c->host_io.alloc(hipHostMallocCoherent));
      c->host_io->done = 0;  // io_seq's values start at 1
    }
    HostIo* h = c->host_io;
    std::memcpy(h->pos, pos, sizeof(dc_pos) * n);
    std::memcpy(h->moves, moves, sizeof(uint16_t) * n);
    const DevPos* dp = reinterpret_cast<const DevPos*>(h->pos);
    const bool flag = n <= kHostFlagBatch && !c->profiling;
    const uint32_t seq = flag ? next_seq(c) : 0u;
    uint32_t* done = flag ? &h->done : nullptr;
    HIP_TRY(c->timed("validate", n, [&] {
      return rules == DC_RULES_REF ? dc::launch_validate_ref(c->stream, dp, h->moves, n, h->verdicts, done, seq)
                                   : dc::launch_validate_fide(c->stream, dp, h->moves, n, h->verdicts, done, seq);
    }));
    const int e = flag ? wait_host_flag(c, done, seq) : sync_ctx(c);
    if (e != DC_SUCCESS) return e;
    std::memcpy(verdicts, h->verdicts, n);
    return DC_SUCCESS;
  }
  HIP_TRY(c->pos.ensure(n));
  HIP_TRY(c->moves.ensure(n));
  HIP_TRY(c->verdicts.ensure(n));
  HIP_TRY(hipMemcpyAsync(c->pos.p, pos, sizeof(dc_pos) * n, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->moves.p, moves, sizeof(uint16_t) * n, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c->timed("validate", n, [&] {
    return rules == DC_RULES_REF ? dc::launch_validate_ref(c->stream, c->pos.p, c->moves.p, n, c->verdicts.p)
                                 : dc::launch_validate_fide(c->stream, c->pos.p, c->moves.p, n, c->verdicts.p);
  }));
  HIP_TRY(hipMemcpyAsync(verdicts, c->verdicts.p, n, hipMemcpyDeviceToHost, c->stream));
  return sync_ctx(c);
}

int dc_apply_batch(dc_ctx* c, uint32_t rules, dc_pos* pos, const uint16_t* moves, uint32_t n, uint8_t* verdicts,
                   uint8_t* info) {
  ENTER(c);
  if (rules > DC_RULES_FIDE || (n && (!pos || !moves || !verdicts))) return DC_EINVAL;
  if (n == 0) return DC_SUCCESS;
  if (live_eligible(c, n)) {
    const int e = live_call(c, true, rules == DC_RULES_FIDE, pos, moves, n, verdicts, info, pos);
    if (e != kLiveDeclined) return e;
  }
  LiveHold live_hold_;  // the launched path (ENTER_WORK)
  if (n <= kHostIoBatch) {  // pinned, read and written in place by the kernel
    if (!c->host_io) {
      HIP_TRY(c->host_io.alloc(hipHostMallocCoherent));
      c->host_io->done = 0;  // io_seq's values start at 1
    }
    HostIo* h = c->host_io;
    std::memcpy(h->pos, pos, sizeof(dc_pos) * n);
    std::memcpy(h->moves, moves, sizeof(uint16_t) * n);
    DevPos* dp = reinterpret_cast<DevPos*>(h->pos);
    const bool flag = n <= kHostFlagBatch && !c->profiling;
    const uint32_t seq = flag ? next_seq(c) : 0u;
    uint32_t* done = flag ? &h->done : nullptr;
    HIP_TRY(c->timed("apply", n, [&] {
      return rules == DC_RULES_REF
                 ? dc::launch_apply_ref(c->stream, dp, h->moves, n, h->verdicts, h->info, done, seq)
                 : dc::launch_apply_fide(c->stream, dp, h->moves, n, h->verdicts, h->info, done, seq);
    }));
    const int e = flag ? wait_host_flag(c, done, seq) : sync_ctx(c);
    if (e != DC_SUCCESS) return e;
    std::memcpy(pos, h->pos, sizeof(dc_pos) * n);
    std::memcpy(verdicts, h->verdicts, n);
    if (info) std::memcpy(info, h->info, n);
    return DC_SUCCESS;
  }
  HIP_TRY(c->pos.ensure(n));
  HIP_TRY(c->moves.ensure(n));
  HIP_TRY(c->verdicts.ensure(n));
  HIP_TRY(c->info.ensure(n));
  HIP_TRY(hipMemcpyAsync(c->pos.p, pos, sizeof(dc_pos) * n, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->moves.p, moves, sizeof(uint16_t) * n, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c->timed("apply", n, [&] {
    return rules == DC_RULES_REF
               ? dc::launch_apply_ref(c->stream, c->pos.p, c->moves.p, n, c->verdicts.p, c->info.p)
               : dc::launch_apply_fide(c->stream, c->pos.p, c->moves.p, n, c->verdicts.p, c->info.p);
  }));
  HIP_TRY(hipMemcpyAsync(pos, c->pos.p, sizeof(dc_pos) * n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(verdicts, c->verdicts.p, n, hipMemcpyDeviceToHost, c->stream));
  if (info) HIP_TRY(hipMemcpyAsync(info, c->info.p, n, hipMemcpyDeviceToHost, c->stream));
  return sync_ctx(c);
}

}  // extern "C"
