// dc_api_san.hip -- what dc_replay_san's bytes say, as text, on the host: the SAN
// token of a move (dc_san_format), a game's PGN movetext (dc_pgn_movetext) and
// the FEN of a position (dc_pos_to_fen).  No context, no device.
#include <cstring>
#include <string>

#include "../../include/dchess.h"

namespace {

void put_square(std::string& s, int sq) {
  s += (char)('a' + (sq & 7));
  s += (char)('1' + (sq >> 3));
}

// The SAN token of one move into s; DC_EINVAL where the byte and the move word
// cannot belong to an accepted move.
int san_token(uint16_t move, uint8_t san, std::string& s) {
  const unsigned kind = san & 7u, promo = (move >> 12) & 7u;
  if (san == 0xFF || kind > 5 || (move & DC_MOVE_OOR)) return DC_EINVAL;
  const int f = move & 63, t = (move >> 6) & 63;
  const bool last = (t >> 3) == 0 || (t >> 3) == 7;
  if (promo > 4 || (kind != 0 && promo) || (kind == 0 && last != (promo != 0))) return DC_EINVAL;
  if (kind == 5 && (f >> 3) == (t >> 3) && ((t & 7) - (f & 7) == 2 || (f & 7) - (t & 7) == 2)) {
    s += (t > f) ? "O-O" : "O-O-O";
  } else {
    if (kind == 0) {
      if (san & DC_SAN_CAPTURE) s += (char)('a' + (f & 7));  // a capturing pawn's file, by rule
    } else {
      s += "PNBRQK"[kind];
      if (san & DC_SAN_FILE) s += (char)('a' + (f & 7));
      if (san & DC_SAN_RANK) s += (char)('1' + (f >> 3));
    }
    if (san & DC_SAN_CAPTURE) s += 'x';
    put_square(s, t);
    if (promo) {
      s += '=';
      s += " NBRQ"[promo];
    }
  }
  if (san & DC_SAN_MATE) s += '#';
  else if (san & DC_SAN_CHECK) s += '+';
  return DC_SUCCESS;
}

// dc_history_append's sizing contract.
int deliver(const std::string& s, char* out, size_t out_cap, size_t* out_len) {
  *out_len = s.size();
  if (out_cap < s.size() + 1) return out_cap ? DC_EINVAL : DC_SUCCESS;
  std::memcpy(out, s.c_str(), s.size() + 1);
  return DC_SUCCESS;
}

}  // namespace

extern "C" {

int dc_san_format(uint16_t move, uint8_t san, char out[8]) {
  if (!out) return DC_EINVAL;
  std::string s;
  const int r = san_token(move, san, s);
  if (r != DC_SUCCESS) return r;
  std::memcpy(out, s.c_str(), s.size() + 1);  // at most 7 characters: "Qh4xe1#", "exd8=Q#"
  return DC_SUCCESS;
}

int dc_pgn_movetext(const uint16_t* moves, const uint8_t* san, uint32_t n_plies, size_t stride, uint32_t first_fullmove,
                    uint8_t first_stm, uint8_t result, char* out, size_t out_cap, size_t* out_len) {
  if ((n_plies && (!moves || !san)) || !out_len || (out_cap && !out) || first_stm > 1 || result >= DC_GO_COUNT)
    return DC_EINVAL;
  if (stride == 0) stride = 1;
  std::string s;
  uint32_t number = first_fullmove;
  unsigned stm = first_stm;  // a skipped ply was not played: the turn stays
  bool first = true;
  for (uint32_t p = 0; p < n_plies; ++p) {
    const uint8_t code = san[(size_t)p * stride];
    if (code == 0xFF) continue;
    if (stm == 0) s += std::to_string(number) + ". ";
    else if (first) s += std::to_string(number) + "... ";
    const int r = san_token(moves[(size_t)p * stride], code, s);
    if (r != DC_SUCCESS) return r;
    s += ' ';
    number += stm;
    stm ^= 1;
    first = false;
  }
  s += result == DC_GO_ONGOING ? "*" : result == DC_GO_WHITE_WINS ? "1-0" : result == DC_GO_BLACK_WINS ? "0-1" : "1/2-1/2";
  return deliver(s, out, out_cap, out_len);
}

int dc_pos_to_fen(const dc_pos* pos, uint32_t halfmove, uint32_t fullmove, char* out, size_t out_cap,
                  size_t* out_len) {
  if (!pos || !out_len || (out_cap && !out) || pos->stm > 1 || pos->ep < -1 || pos->ep > 63) return DC_EINVAL;
  int8_t cells[64];
  const int r = dc_pos_to_cells(pos, cells, nullptr);
  if (r != DC_SUCCESS) return r;
  std::string s;
  for (int x = 7; x >= 0; --x) {
    int run = 0;
    for (int y = 0; y < 8; ++y) {
      const int8_t c = cells[8 * x + y];
      if (c == DC_CELL_EMPTY) {
        ++run;
        continue;
      }
      if ((c & 7) > 5) return DC_EUNSUPPORTED;  // OTHER has no FEN letter
      if (run) s += (char)('0' + run);
      run = 0;
      s += ((c >> 3) ? "pnbrqk" : "PNBRQK")[c & 7];
    }
    if (run) s += (char)('0' + run);
    if (x) s += '/';
  }
  s += pos->stm ? " b " : " w ";
  if (pos->castle & 15) {
    for (int k = 0; k < 4; ++k)
      if (pos->castle & (1 << k)) s += "KQkq"[k];
  } else {
    s += '-';
  }
  s += ' ';
  if (pos->ep >= 0) put_square(s, pos->ep);
  else s += '-';
  s += ' ' + std::to_string(halfmove) + ' ' + std::to_string(fullmove);
  return deliver(s, out, out_cap, out_len);
}

}  // extern "C"
