// dc_api_multi.hip -- the one-process multi-GPU entry points over RCCL
// (dc_multi_perft, dc_multi_replay) and the replay shard layout they share.
#include <rccl/rccl.h>

#include <cstring>
#include <thread>

#include "dc_ctx.h"

extern "C" {

// One process, several GPUs: a host thread per device computes its shard of
// the frontier, then one grouped ncclAllReduce(ncclUint64, ncclSum) over the
// per-device divide[] vectors combines them over xGMI.
int dc_multi_perft(const int* devices, int n_devices, uint32_t rules, const dc_pos* pos, uint32_t depth,
                   uint64_t* divide, uint16_t* root_moves, uint32_t* n_root, uint64_t* total) {
  if (!devices || n_devices <= 0 || !pos || !total) return DC_EINVAL;
  std::vector<dc_ctx*> ctx(n_devices, nullptr);
  for (int i = 0; i < n_devices; ++i) {
    int r = dc_ctx_create(devices[i], &ctx[i]);
    if (r != DC_SUCCESS) {
      for (auto* x : ctx)
        if (x) dc_ctx_destroy(x);
      return r;
    }
  }
  const u32 split = depth >= 5 ? 3 : (depth >= 3 ? depth - 2 : 1);
  std::vector<int> rc(n_devices, DC_SUCCESS);
  std::vector<uint32_t> nroot(n_devices, 0);
  std::vector<uint16_t> rm(256);
  std::vector<std::thread> th;
  for (int i = 0; i < n_devices; ++i)
    th.emplace_back([&, i] {
      uint64_t tot = 0;
      rc[i] = dc_perft_shard(ctx[i], rules, pos, depth, split, (u32)i, (u32)n_devices, nullptr,
                             i == 0 ? rm.data() : nullptr, &nroot[i], &tot);
    });
  for (auto& t : th) t.join();
  int result = DC_SUCCESS;
  for (int r : rc)
    if (r != DC_SUCCESS) result = r;
  std::vector<u64> div(256, 0);
  // every shard rebuilds the same root moves: a disagreement is a bug, never summed over
  for (int i = 1; i < n_devices && result == DC_SUCCESS; ++i)
    if (nroot[i] != nroot[0]) result = DC_EHIP;
  if (result == DC_SUCCESS && depth > 0) {
    std::vector<ncclComm_t> comms(n_devices);
    if (ncclCommInitAll(comms.data(), n_devices, devices) != ncclSuccess) {
      result = DC_ERCCL;
    } else {
      if (ncclGroupStart() != ncclSuccess) result = DC_ERCCL;
      for (int i = 0; i < n_devices && result == DC_SUCCESS; ++i) {
        if (hipSetDevice(devices[i]) != hipSuccess) result = DC_EHIP;
        else if (ncclAllReduce(ctx[i]->res.p->divide, ctx[i]->res.p->divide, nroot[0], ncclUint64, ncclSum, comms[i],
                               ctx[i]->stream) != ncclSuccess)
          result = DC_ERCCL;
      }
      if (ncclGroupEnd() != ncclSuccess) result = DC_ERCCL;
      for (int i = 0; i < n_devices; ++i) {
        (void)hipSetDevice(devices[i]);
        if (hipStreamSynchronize(ctx[i]->stream) != hipSuccess) result = DC_EHIP;
      }
      if (result == DC_SUCCESS) {
        (void)hipSetDevice(devices[0]);
        if (hipMemcpy(div.data(), ctx[0]->res.p->divide, nroot[0] * sizeof(u64), hipMemcpyDeviceToHost) != hipSuccess)
          result = DC_EHIP;
      }
      for (auto& cm : comms) ncclCommDestroy(cm);
    }
  }
  if (result == DC_SUCCESS) {
    u64 t = 0;
    if (depth == 0) t = 1;
    for (u32 i = 0; i < nroot[0]; ++i) {
      t += div[i];
      if (divide) divide[i] = div[i];
    }
    if (depth == 1) {
      t = nroot[0];
      if (divide)
        for (u32 i = 0; i < nroot[0]; ++i) divide[i] = 1;
    }
    if (root_moves) std::copy(rm.begin(), rm.begin() + nroot[0], root_moves);
    if (n_root) *n_root = nroot[0];
    *total = t;
  }
  for (auto* x : ctx) dc_ctx_destroy(x);
  return result;
}


// ---------------------------------------------------------- multi-GPU replay
// Contiguous game-id ranges of whole 64-game bitmap words, so shard s's accept
// bitmap [n_plies][count/64] is a word-column block of the global ply-major
// bitmap [n_plies][ceil(n_games/64)], at word offset first/64.
int dc_replay_shard_range(uint64_t n_games, uint32_t shard, uint32_t n_shards, uint64_t* first, uint64_t* count) {
  if (!first || !count || n_shards == 0 || shard >= n_shards) return DC_EINVAL;
  const u64 words = (n_games + 63) / 64, per = (words + n_shards - 1) / n_shards;
  const u64 lo = std::min<u64>(n_games, std::min<u64>(words, (u64)shard * per) * 64);
  const u64 hi = std::min<u64>(n_games, std::min<u64>(words, (u64)(shard + 1) * per) * 64);
  *first = lo;
  *count = hi > lo ? hi - lo : 0;
  return DC_SUCCESS;
}

// One process, n_devices GPUs: device i generates (dc_gen_games_device) and
// replays (dc_replay_device) shard i of the game ids; the per-shard bitmaps
// go to device 0 with one ncclGather over xGMI (rccl.h:745) and from there to
// the host; the five counters are folded on the host (sums mod 2^64, xor).
// The gather layout of the replay shards (dc_replay_shard_range's contract):
// shard i's bitmap, padded to `per` words per ply row, is block i of
// `gathered` ([n_shards][n_plies][per]); its first ceil(count_i / 64) words of
// each row go to word first_i / 64 of the whole batch's row.
int dc_replay_scatter_shards(uint64_t n_games, uint32_t n_shards, uint32_t n_plies, const uint64_t* gathered,
                             uint64_t* bitmap) {
  if (n_shards == 0 || (n_games && n_plies && (!gathered || !bitmap))) return DC_EINVAL;
  const u64 words = (n_games + 63) / 64, per = (words + n_shards - 1) / n_shards;
  for (u32 i = 0; i < n_shards; ++i) {
    uint64_t first = 0, cnt = 0;
    const int r = dc_replay_shard_range(n_games, i, n_shards, &first, &cnt);
    if (r != DC_SUCCESS) return r;
    const u64 w_r = (cnt + 63) / 64;
    for (u32 p = 0; p < n_plies && w_r; ++p)
      std::memcpy(bitmap + (size_t)p * words + first / 64, gathered + ((size_t)i * n_plies + p) * per, w_r * 8);
  }
  return DC_SUCCESS;
}

int dc_multi_replay(const int* devices, int n_devices, uint32_t rules, uint64_t seed, uint64_t n_games,
                    uint32_t n_plies, uint32_t noise_per_256, uint64_t* bitmap, dc_replay_stats* stats) {
  if (!devices || n_devices <= 0 || rules > DC_RULES_FIDE || noise_per_256 > 256) return DC_EINVAL;
  const u64 words = (n_games + 63) / 64, per = (words + n_devices - 1) / n_devices;
  if (per * 64 > 0xFFFFFFFFull) return DC_EUNSUPPORTED;  // a shard's game count is a u32
  std::vector<dc_ctx*> ctx(n_devices, nullptr);
  for (int i = 0; i < n_devices; ++i) {
    int r = dc_ctx_create(devices[i], &ctx[i]);
    if (r != DC_SUCCESS) {
      for (auto* x : ctx)
        if (x) dc_ctx_destroy(x);
      return r;
    }
  }
  const size_t shard_words = (size_t)per * n_plies;  // every shard's bitmap padded to `per` words per ply
  std::vector<int> rc(n_devices, DC_SUCCESS);
  std::vector<dc_replay_stats> st(n_devices);
  std::vector<void*> d_moves(n_devices, nullptr), d_bm(n_devices, nullptr);
  void* d_all = nullptr;  // device 0: the gathered [n_devices][n_plies][per]
  std::vector<std::thread> th;
  for (int i = 0; i < n_devices; ++i)
    th.emplace_back([&, i] {
      uint64_t first = 0, cnt = 0;
      int r = dc_replay_shard_range(n_games, (u32)i, (u32)n_devices, &first, &cnt);
      if (r == DC_SUCCESS) r = dc_device_alloc(ctx[i], std::max<size_t>((size_t)cnt * n_plies * 2, 2), &d_moves[i]);
      if (r == DC_SUCCESS) r = dc_device_alloc(ctx[i], std::max<size_t>(shard_words * 8, 8), &d_bm[i]);
      if (r == DC_SUCCESS && i == 0 && bitmap)
        r = dc_device_alloc(ctx[i], std::max<size_t>(shard_words * 8 * n_devices, 8), &d_all);
      if (r == DC_SUCCESS && hipMemsetAsync(d_bm[i], 0, shard_words * 8, ctx[i]->stream) != hipSuccess) r = DC_EHIP;
      if (r == DC_SUCCESS)
        r = dc_gen_games_device(ctx[i], rules, seed, first, (u32)cnt, n_plies, noise_per_256,
                                static_cast<uint16_t*>(d_moves[i]));
      // the shard's bitmap rows are `per` words apart: replay into a dense
      // [n_plies][cnt/64] block, then spread the rows (dense = padded when full)
      if (r == DC_SUCCESS) {
        const u64 w_r = (cnt + 63) / 64;
        void* dense = d_bm[i];
        if (w_r != per && cnt) r = dc_device_alloc(ctx[i], (size_t)w_r * n_plies * 8, &dense);
        if (r == DC_SUCCESS)
          r = dc_replay_device(ctx[i], rules, nullptr, static_cast<uint16_t*>(d_moves[i]), (u32)cnt, n_plies,
                               static_cast<uint64_t*>(dense), nullptr, &st[i]);
        if (r == DC_SUCCESS && dense != d_bm[i]) {
          if (hipMemcpy2DAsync(d_bm[i], per * 8, dense, w_r * 8, w_r * 8, n_plies, hipMemcpyDeviceToDevice,
                               ctx[i]->stream) != hipSuccess)
            r = DC_EHIP;
          else
            r = sync_ctx(ctx[i]);
          dc_device_free(ctx[i], dense);
        }
      }
      rc[i] = r;
    });
  for (auto& t : th) t.join();
  int result = DC_SUCCESS;
  for (int r : rc)
    if (r != DC_SUCCESS) result = r;
  if (result == DC_SUCCESS && bitmap && n_plies && words) {
    std::vector<ncclComm_t> comms(n_devices);
    if (ncclCommInitAll(comms.data(), n_devices, devices) != ncclSuccess) {
      result = DC_ERCCL;
    } else {
      if (ncclGroupStart() != ncclSuccess) result = DC_ERCCL;
      for (int i = 0; i < n_devices && result == DC_SUCCESS; ++i) {
        if (hipSetDevice(devices[i]) != hipSuccess) result = DC_EHIP;
        else if (ncclGather(d_bm[i], i == 0 ? d_all : nullptr, shard_words, ncclUint64, 0, comms[i], ctx[i]->stream) !=
                 ncclSuccess)
          result = DC_ERCCL;
      }
      if (ncclGroupEnd() != ncclSuccess) result = DC_ERCCL;
      for (int i = 0; i < n_devices; ++i) {
        (void)hipSetDevice(devices[i]);
        if (hipStreamSynchronize(ctx[i]->stream) != hipSuccess) result = DC_EHIP;
      }
      for (auto& cm : comms) ncclCommDestroy(cm);
    }
    // device 0 -> host, then each shard's rows to word offset first_i / 64 of
    // every ply row (dc_replay_scatter_shards: the layout is host-tested)
    if (result == DC_SUCCESS) {
      std::vector<u64> all((size_t)n_devices * shard_words);
      (void)hipSetDevice(devices[0]);
      if (hipMemcpy(all.data(), d_all, all.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) result = DC_EHIP;
      else result = dc_replay_scatter_shards(n_games, (u32)n_devices, n_plies, reinterpret_cast<const uint64_t*>(all.data()), bitmap);
    }
  }
  if (result == DC_SUCCESS && stats) {
    dc_replay_stats t{0, 0, 0, 0, 0};
    for (auto& x : st) {
      t.validated += x.validated;
      t.accepted += x.accepted;
      t.rejected += x.rejected;
      t.digest_sum += x.digest_sum;
      t.digest_xor ^= x.digest_xor;
    }
    *stats = t;
  }
  for (int i = 0; i < n_devices; ++i) {
    if (d_moves[i]) dc_device_free(ctx[i], d_moves[i]);
    if (d_bm[i]) dc_device_free(ctx[i], d_bm[i]);
  }
  if (d_all) dc_device_free(ctx[0], d_all);
  for (auto* x : ctx) dc_ctx_destroy(x);
  return result;
}
}  // extern "C"
