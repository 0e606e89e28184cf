// dc_api_legal.hip -- dc_legal_moves_batch / dc_legal_moves_batch_device.
#include <cstring>

#include "dc_ctx.h"
#include "dc_movegen.h"

// dc_legal_moves_batch of at most one block (the one-position call of a front
// end): positions in, offsets / status / total / moves out, all in one pinned
// block the fused kernel reads and writes in place.  A batch whose moves do
// not fit kLegalIoMoves takes the three-launch path through device buffers.
// (Defined here, not in dc_ctx.h: its size is dc_movegen.h's kLegalBlock.)
constexpr uint32_t kLegalIoMoves = 256 * 256;
struct LegalIo {
  dc_pos pos[dc::kLegalBlock];
  uint32_t offsets[dc::kLegalBlock + 1];
  uint8_t status[dc::kLegalBlock];
  uint64_t total;  // also the three-launch path's total (k_legal_scan stores it here)
  uint32_t done;
  alignas(16) uint16_t moves[kLegalIoMoves];
};

extern "C" {

// ============================================================= legal moves
static int legal_io_ensure(dc_ctx* c) {
  if (c->legal_io) return DC_SUCCESS;
  HIP_TRY(c->legal_io.alloc(hipHostMallocCoherent));
  c->legal_io->done = 0;  // io_seq's values start at 1
  c->legal_io->total = 0;
  return DC_SUCCESS;
}

// n <= kLegalBlock: the fused kernel on the given buffers (device memory, or
// the pinned LegalIo); the total comes back through legal_io->total.
static int legal_small(dc_ctx* c, uint32_t rules, const DevPos* pos, uint32_t n, u32* offsets, uint8_t* status,
                       uint16_t* moves, uint32_t cap, u64* total) {
  LegalIo* h = c->legal_io;
  const bool flag = !c->profiling;
  const uint32_t seq = flag ? next_seq(c) : 0u;
  uint32_t* done = flag ? &h->done : nullptr;
  HIP_TRY(c->timed("legal_small", n, [&] {
    return dc::launch_legal_small(c->stream, rules, pos, n, offsets, status, moves, cap,
                                  reinterpret_cast<u64*>(&h->total), done, seq);
  }));
  const int e = flag ? wait_host_flag(c, done, seq) : sync_ctx(c);
  if (e != DC_SUCCESS) return e;
  *total = __atomic_load_n(&h->total, __ATOMIC_ACQUIRE);
  return DC_SUCCESS;
}

// Any n, device buffers: counts, status and block-local offsets, then the scan
// of the block sums; returns with the 64-bit total on the host.
static int legal_count_scan(dc_ctx* c, uint32_t rules, const DevPos* d_pos, uint32_t n, u32* d_offsets,
                            uint8_t* d_status, u64* total) {
  const u32 nb = (n + dc::kLegalBlock - 1) / dc::kLegalBlock;
  HIP_TRY(c->legal_bsum.ensure(nb));
  HIP_TRY(c->legal_bbase.ensure(nb));
  HIP_TRY(c->timed("legal_count", n, [&] {
    return dc::launch_legal_count(c->stream, rules, d_pos, n, d_offsets, d_status, c->legal_bsum.p);
  }));
  HIP_TRY(c->timed("legal_scan", nb, [&] {
    return dc::launch_legal_scan(c->stream, c->legal_bsum.p, nb, c->legal_bbase.p, d_offsets + n,
                                 reinterpret_cast<u64*>(&c->legal_io->total));
  }));
  const int e = sync_ctx(c);
  if (e != DC_SUCCESS) return e;
  *total = __atomic_load_n(&c->legal_io->total, __ATOMIC_ACQUIRE);
  return DC_SUCCESS;
}

// The second half: the moves (d_moves != nullptr: `total` of them fit) with the
// final offsets, or the final offsets alone.  Enqueued, not synchronised.
static int legal_finish(dc_ctx* c, uint32_t rules, const DevPos* d_pos, uint32_t n, u32* d_offsets,
                        uint16_t* d_moves, uint32_t total) {
  if (d_moves) {
    HIP_TRY(c->timed("legal_emit", total, [&] {
      return dc::launch_legal_emit(c->stream, rules, d_pos, n, d_offsets, c->legal_bsum.p, c->legal_bbase.p, d_moves,
                                   total);
    }));
  } else {
    HIP_TRY(c->timed("legal_fixup", n, [&] {
      return dc::launch_legal_fixup(c->stream, d_offsets, n, c->legal_bbase.p);
    }));
  }
  return DC_SUCCESS;
}

int dc_legal_moves_batch_device(dc_ctx* c, uint32_t rules, const dc_pos* d_pos, uint32_t n, uint32_t* d_offsets,
                                uint8_t* d_status, uint16_t* d_moves, uint32_t moves_cap, uint32_t* total) {
  ENTER_WORK(c);
  if (rules > DC_RULES_FIDE || (n && (!d_pos || !d_offsets))) return DC_EINVAL;
  if (total) *total = 0;
  if (n == 0) {
    if (d_offsets) {
      HIP_TRY(hipMemsetAsync(d_offsets, 0, sizeof(uint32_t), c->stream));
      return sync_ctx(c);
    }
    return DC_SUCCESS;
  }
  int e = legal_io_ensure(c);
  if (e != DC_SUCCESS) return e;
  const bool sizing = !d_moves || moves_cap == 0;
  const DevPos* dp = reinterpret_cast<const DevPos*>(d_pos);
  u64 t = 0;
  if (n <= dc::kLegalBlock) {
    e = legal_small(c, rules, dp, n, d_offsets, d_status, sizing ? nullptr : d_moves, sizing ? 0u : moves_cap, &t);
    if (e != DC_SUCCESS) return e;
    if (total) *total = (uint32_t)t;
    return (!sizing && t > moves_cap) ? DC_EINVAL : DC_SUCCESS;
  }
  e = legal_count_scan(c, rules, dp, n, d_offsets, d_status, &t);
  if (e != DC_SUCCESS) return e;
  if (t > 0xFFFFFFFFull) return DC_EUNSUPPORTED;
  if (total) *total = (uint32_t)t;
  const bool fill = !sizing && t <= moves_cap;
  e = legal_finish(c, rules, dp, n, d_offsets, fill ? d_moves : nullptr, (uint32_t)t);
  if (e != DC_SUCCESS) return e;
  e = sync_ctx(c);
  if (e != DC_SUCCESS) return e;
  return (sizing || fill) ? DC_SUCCESS : DC_EINVAL;
}

int dc_legal_moves_batch(dc_ctx* c, uint32_t rules, const dc_pos* pos, uint32_t n, uint32_t* offsets, uint8_t* status,
                         uint16_t* moves, uint32_t moves_cap, uint32_t* total) {
  ENTER_WORK(c);
  if (rules > DC_RULES_FIDE || (n && (!pos || !offsets))) return DC_EINVAL;
  if (total) *total = 0;
  if (n == 0) {
    if (offsets) offsets[0] = 0;
    return DC_SUCCESS;
  }
  int e = legal_io_ensure(c);
  if (e != DC_SUCCESS) return e;
  const bool sizing = !moves || moves_cap == 0;
  u64 t = 0;
  if (n <= dc::kLegalBlock) {  // pinned, read and written in place by the kernel
    LegalIo* h = c->legal_io;
    std::memcpy(h->pos, pos, sizeof(dc_pos) * n);
    const uint32_t kcap = sizing ? 0u : std::min(moves_cap, kLegalIoMoves);
    e = legal_small(c, rules, reinterpret_cast<const DevPos*>(h->pos), n, h->offsets, h->status,
                    sizing ? nullptr : h->moves, kcap, &t);
    if (e != DC_SUCCESS) return e;
    std::memcpy(offsets, h->offsets, sizeof(uint32_t) * ((size_t)n + 1));
    if (status) std::memcpy(status, h->status, n);
    if (total) *total = (uint32_t)t;
    if (sizing) return DC_SUCCESS;
    if (t > moves_cap) return DC_EINVAL;
    if (t <= kcap) {
      std::memcpy(moves, h->moves, sizeof(uint16_t) * (size_t)t);
      return DC_SUCCESS;
    }
    // more moves than the pinned block holds: the three-launch path
  }
  HIP_TRY(c->pos.ensure(n));
  HIP_TRY(c->legal_off.ensure((size_t)n + 1));
  HIP_TRY(c->legal_status.ensure(n));
  HIP_TRY(hipMemcpyAsync(c->pos.p, pos, sizeof(dc_pos) * n, hipMemcpyHostToDevice, c->stream));
  e = legal_count_scan(c, rules, c->pos.p, n, c->legal_off.p, c->legal_status.p, &t);
  if (e != DC_SUCCESS) return e;
  if (t > 0xFFFFFFFFull) return DC_EUNSUPPORTED;
  if (total) *total = (uint32_t)t;
  const bool fill = !sizing && t <= moves_cap;
  if (fill) HIP_TRY(c->legal_moves.ensure(std::max<size_t>((size_t)t, 1)));
  e = legal_finish(c, rules, c->pos.p, n, c->legal_off.p, fill ? c->legal_moves.p : nullptr, (uint32_t)t);
  if (e != DC_SUCCESS) return e;
  HIP_TRY(hipMemcpyAsync(offsets, c->legal_off.p, sizeof(uint32_t) * ((size_t)n + 1), hipMemcpyDeviceToHost,
                         c->stream));
  if (status) HIP_TRY(hipMemcpyAsync(status, c->legal_status.p, n, hipMemcpyDeviceToHost, c->stream));
  if (fill && t)
    HIP_TRY(hipMemcpyAsync(moves, c->legal_moves.p, sizeof(uint16_t) * (size_t)t, hipMemcpyDeviceToHost, c->stream));
  e = sync_ctx(c);
  if (e != DC_SUCCESS) return e;
  return (sizing || fill) ? DC_SUCCESS : DC_EINVAL;
}

}  // extern "C"
