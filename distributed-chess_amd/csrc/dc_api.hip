// dc_api.hip -- implementation of include/dchess.h (host side of the engine):
// this unit holds the context's life cycle, device memory and the layout
// adapters; dc_api_validate, _legal, _replay, _txsig, _perft and _multi hold
// the entry points of their subsystems, all around the context of dc_ctx.h.
//
// The context owns the stream, grow-only device buffers and HIP-event kernel
// timing; the units drive the kernels of dc_moves, dc_perft, dc_hash, dc_txsig
// and dc_movegen.  No rule is ever evaluated on the host: every verdict, count
// and state update comes from a gfx950 kernel, and every entry point fails
// with DC_ENODEV when no device is usable -- there is no CPU fallback.
#include <cstring>

#include "dc_ctx.h"

static_assert(sizeof(dc_pos) == sizeof(DevPos), "dc_pos / DevPos layout");

std::atomic<uint64_t> dcapi::g_alloc_epoch{0};

// ================================================================ context
extern "C" {

int dc_version(void) { return 101; }  // 101: the *_starts calls

const char* dc_strerror(int s) {
  switch (s) {
    case DC_SUCCESS: return "success";
    case DC_EINVAL: return "invalid argument";
    case DC_EHIP: return "HIP runtime error";
    case DC_ENOMEM: return "out of memory";
    case DC_ENODEV: return "no usable gfx950 device";
    case DC_ERCCL: return "RCCL error";
    case DC_EUNSUPPORTED: return "unsupported request";
  }
  return "unknown status";
}

const char* dc_verdict_message(uint8_t v) {
  switch (v) {
    case DC_V_OK: return "";
    case DC_V_NO_PIECE: return "No piece at the source location";       // chess.rs:104-106
    case DC_V_WRONG_TURN: return "It's not this piece's turn to move";  // chess.rs:113-115
    case DC_V_ILLEGAL: return "Invalid move for the piece";             // chess.rs:119-121
    case DC_V_OOR: return "Position out of range";
  }
  return "Unknown verdict";
}

int dc_ctx_create(int device, dc_ctx** out) {
  if (!out) return DC_EINVAL;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return DC_ENODEV;
  if (device < 0 || device >= n) return DC_ENODEV;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return DC_ENODEV;
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return DC_ENODEV;  // code objects are gfx950-only
  HIP_TRY(hipSetDevice(device));
  dc_ctx* c = new dc_ctx();
  c->device = device;
  if (hipStreamCreateWithFlags(&c->stream.h, hipStreamNonBlocking) != hipSuccess) {
    LiveHold hold;
    delete c;
    return DC_EHIP;
  }
  *out = c;
  return DC_SUCCESS;
}

int dc_ctx_destroy(dc_ctx* c) {
  if (!c) return DC_EINVAL;
  (void)hipSetDevice(c->device);
  dcapi::live_retire(c);
  (void)hipStreamSynchronize(c->stream);
  LiveHold hold;  // one hold for the whole teardown: the frees wait for every stream
  delete c;
  return DC_SUCCESS;
}

int dc_ctx_device(const dc_ctx* c) { return c ? c->device : -1; }
void* dc_ctx_stream(dc_ctx* c) { return c ? (void*)c->stream : nullptr; }

int dc_ctx_set_profiling(dc_ctx* c, int enable) {
  if (!c) return DC_EINVAL;
  c->profiling = enable != 0;
  return DC_SUCCESS;
}

int dc_ctx_kernel_stats(dc_ctx* c, const char* kernel, dc_kernel_stats* out) {
  if (!c || !kernel || !out) return DC_EINVAL;
  auto it = c->stats.find(kernel);
  if (it == c->stats.end()) {
    *out = dc_kernel_stats{0, 0.0, 0};
  } else {
    out->launches = it->second.launches;
    out->total_ms = it->second.ms;
    out->units = it->second.units;
  }
  return DC_SUCCESS;
}

int dc_ctx_reset_stats(dc_ctx* c) {
  if (!c) return DC_EINVAL;
  c->stats.clear();
  return DC_SUCCESS;
}

int dc_device_alloc(dc_ctx* c, size_t bytes, void** d_ptr) {
  ENTER_WORK(c);
  if (!d_ptr) return DC_EINVAL;
  *d_ptr = nullptr;
  HIP_TRY(hipMalloc(d_ptr, std::max<size_t>(bytes, 1)));
  return DC_SUCCESS;
}

int dc_device_free(dc_ctx* c, void* d_ptr) {
  ENTER_WORK(c);
  if (d_ptr) HIP_TRY(hipFree(d_ptr));
  return DC_SUCCESS;
}

int dc_memcpy_h2d(dc_ctx* c, void* d_dst, const void* src, size_t bytes) {
  ENTER_WORK(c);
  if (bytes && (!d_dst || !src)) return DC_EINVAL;
  if (bytes) HIP_TRY(hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, c->stream));
  return sync_ctx(c);
}

int dc_memcpy_d2h(dc_ctx* c, void* dst, const void* d_src, size_t bytes) {
  ENTER_WORK(c);
  if (bytes && (!dst || !d_src)) return DC_EINVAL;
  if (bytes) HIP_TRY(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, c->stream));
  return sync_ctx(c);
}

int dc_ctx_synchronize(dc_ctx* c) {
  ENTER_WORK(c);
  return sync_ctx(c);
}

// ================================================================ adapters
// Cell kind (P N B R Q K X) -> ABI kind code (P=1 N=2 B=5 R=6 Q=7 K=3 X=4).
static const int kCellToCode[7] = {1, 2, 5, 6, 7, 3, 4};
static const int kCodeToCell[8] = {-1, 0, 1, 5, 6, 2, 3, 4};

int dc_startpos(dc_pos* out) {
  if (!out) return DC_EINVAL;
  std::memset(out, 0, sizeof *out);
  out->bb[0] = dc::kStartB0;
  out->bb[1] = dc::kStartB1;
  out->bb[2] = dc::kStartB2;
  out->bb[3] = dc::kStartB3;
  out->stm = 0;
  out->castle = 15;
  out->ep = -1;
  return DC_SUCCESS;
}

int dc_pos_from_cells(const int8_t cells[64], uint8_t turn, dc_pos* out) {
  if (!cells || !out || turn > 1) return DC_EINVAL;  // Color::from_i32 panics otherwise (chess.rs:110)
  dc_pos p;
  std::memset(&p, 0, sizeof p);
  for (int s = 0; s < 64; ++s) {
    const int8_t c = cells[s];
    if (c == DC_CELL_EMPTY) continue;
    if (c < 0 || (c >> 3) > 1 || (c & 7) > 6) return DC_EINVAL;  // colour outside {0,1} is not representable
    const uint64_t m = 1ull << s;
    const int code = kCellToCode[c & 7];
    if (c >> 3) p.bb[0] |= m;
    if (code & 1) p.bb[1] |= m;
    if (code & 2) p.bb[2] |= m;
    if (code & 4) p.bb[3] |= m;
  }
  p.stm = turn;
  p.castle = 0;
  p.ep = -1;
  *out = p;
  return DC_SUCCESS;
}

int dc_pos_to_cells(const dc_pos* pos, int8_t cells[64], uint8_t* turn) {
  if (!pos || !cells) return DC_EINVAL;
  for (int s = 0; s < 64; ++s) {
    const int code = (int)(((pos->bb[1] >> s) & 1) | (((pos->bb[2] >> s) & 1) << 1) | (((pos->bb[3] >> s) & 1) << 2));
    if (code == 0) {
      cells[s] = DC_CELL_EMPTY;
      continue;
    }
    cells[s] = (int8_t)(((pos->bb[0] >> s) & 1) * 8 + kCodeToCell[code]);
  }
  if (turn) *turn = pos->stm;
  return DC_SUCCESS;
}

int dc_pos_from_fen(const char* fen, dc_pos* out) {
  if (!fen || !out) return DC_EINVAL;
  int8_t cells[64];
  std::memset(cells, DC_CELL_EMPTY, sizeof cells);
  int x = 7, y = 0;
  const char* s = fen;
  for (; *s && *s != ' '; ++s) {
    if (*s == '/') {
      if (y != 8 || x == 0) return DC_EINVAL;
      --x;
      y = 0;
      continue;
    }
    if (*s >= '1' && *s <= '8') {
      y += *s - '0';
      if (y > 8) return DC_EINVAL;
      continue;
    }
    static const char* kinds = "pnbrqk";
    const char* k = std::strchr(kinds, *s | 0x20);
    if (!k || y > 7) return DC_EINVAL;
    cells[8 * x + y] = (int8_t)(((*s >= 'a') ? 8 : 0) + (k - kinds));
    ++y;
  }
  if (x != 0 || y != 8) return DC_EINVAL;
  while (*s == ' ') ++s;
  uint8_t stm = 0;
  if (*s == 'b') stm = 1;
  else if (*s != 'w') return DC_EINVAL;
  ++s;
  while (*s == ' ') ++s;
  uint8_t castle = 0;
  for (; *s && *s != ' '; ++s) {
    switch (*s) {
      case 'K': castle |= 1; break;
      case 'Q': castle |= 2; break;
      case 'k': castle |= 4; break;
      case 'q': castle |= 8; break;
      case '-': break;
      default: return DC_EINVAL;
    }
  }
  while (*s == ' ') ++s;
  int8_t ep = -1;
  if (*s >= 'a' && *s <= 'h' && s[1] >= '1' && s[1] <= '8') ep = (int8_t)((s[1] - '1') * 8 + (s[0] - 'a'));
  int r = dc_pos_from_cells(cells, stm, out);
  if (r != DC_SUCCESS) return r;
  out->castle = castle;
  out->ep = ep;
  return DC_SUCCESS;
}

uint16_t dc_move_pack(uint32_t fx, uint32_t fy, uint32_t tx, uint32_t ty) {
  if (fx >= 8 || fy >= 8 || tx >= 8 || ty >= 8) return (uint16_t)DC_MOVE_OOR;
  return (uint16_t)((8 * fx + fy) | ((8 * tx + ty) << 6));
}

int dc_move_pack_batch(const uint32_t* actions, uint32_t n, uint16_t* moves) {
  if (n && (!actions || !moves)) return DC_EINVAL;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t* a = actions + (size_t)4 * i;
    moves[i] = dc_move_pack(a[0], a[1], a[2], a[3]);
  }
  return DC_SUCCESS;
}

}  // extern "C"
