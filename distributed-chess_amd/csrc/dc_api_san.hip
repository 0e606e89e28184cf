// dc_api_san.hip -- what dc_replay_san's bytes say, as text, on the host: the SAN
// token of a move (dc_san_format), a game's PGN movetext (dc_pgn_movetext) and
// the FEN of a position (dc_pos_to_fen); and the way back as far as the host
// goes: a SAN token or a game's movetext as token words (dc_san_parse,
// dc_pgn_parse_movetext) for dc_san_resolve.  No context, no device.
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

// ---------------------------------------------------------------- input
enum : uint32_t {
  TOK_FILE_GIVEN = 1u << 12,
  TOK_RANK_GIVEN = 1u << 16,
  TOK_OO = 1u << 20,
  TOK_OOO = 1u << 21,
  TOK_X = 1u << 22,
  TOK_CHECK = 1u << 23,
  TOK_MATE = 1u << 24
};

bool is_file(char ch) { return ch >= 'a' && ch <= 'h'; }
bool is_rank(char ch) { return ch >= '1' && ch <= '8'; }
bool is_space(char ch) { return ch == ' ' || ch == '\t' || ch == '\n' || ch == '\r' || ch == '\v' || ch == '\f'; }

// One SAN token from text[0, len); false where it is none.
bool parse_san(const char* p, size_t len, uint32_t& token) {
  size_t i = 0;
  uint32_t tok = 0;
  auto at = [&](size_t k) { return k < len ? p[k] : '\0'; };
  if (at(0) == 'O' || at(0) == '0') {
    auto o = [&](size_t k) { return at(k) == 'O' || at(k) == '0'; };
    if (at(1) != '-' || !o(2)) return false;
    if (at(3) == '-' && o(4)) {
      tok = TOK_OOO;
      i = 5;
    } else {
      tok = TOK_OO;
      i = 3;
    }
  } else {
    uint32_t kind = 0;
    const char* piece = at(0) ? std::strchr("NBRQK", at(0)) : nullptr;
    if (piece) {
      kind = (uint32_t)(piece - "NBRQK") + 1;
      ++i;
    }
    int file = -1, rank = -1;
    if (is_file(at(i))) file = at(i++) - 'a';
    if (is_rank(at(i))) rank = at(i++) - '1';
    bool takes = false;
    if (at(i) == 'x') {
      takes = true;
      ++i;
    }
    int t;
    if (is_file(at(i)) && is_rank(at(i + 1))) {  // what came before is the origin
      t = 8 * (at(i + 1) - '1') + (at(i) - 'a');
      i += 2;
    } else if (!takes && file >= 0 && rank >= 0) {  // ... or it was the target itself
      t = 8 * rank + file;
      file = rank = -1;
    } else {
      return false;
    }
    tok = (uint32_t)t | (kind << 6) | (takes ? TOK_X : 0u);
    if (file >= 0) tok |= TOK_FILE_GIVEN | ((uint32_t)file << 13);
    if (rank >= 0) tok |= TOK_RANK_GIVEN | ((uint32_t)rank << 17);
    if (at(i) == '=') {
      const char* pr = at(i + 1) ? std::strchr("NBRQ", at(i + 1)) : nullptr;
      if (!pr || kind != 0) return false;  // a piece does not promote
      tok |= ((uint32_t)(pr - "NBRQ") + 1) << 9;
      i += 2;
    }
  }
  if (at(i) == '+') {
    tok |= TOK_CHECK;
    ++i;
  } else if (at(i) == '#') {
    tok |= TOK_MATE;
    ++i;
  }
  while (at(i) == '!' || at(i) == '?') ++i;
  if (i != len) return false;
  token = tok;
  return true;
}

}  // namespace

extern "C" {

int dc_san_parse(const char* text, size_t len, uint32_t* token) {
  if (!text || !token || len == 0) return DC_EINVAL;
  uint32_t tok;
  if (!parse_san(text, len, tok)) return DC_EINVAL;
  *token = tok;
  return DC_SUCCESS;
}

int dc_pgn_parse_movetext(const char* text, size_t len, uint32_t* tokens, size_t stride, uint32_t cap,
                          uint32_t* n_tokens, uint8_t* result, uint32_t* first_fullmove, uint8_t* first_stm,
                          size_t* consumed) {
  if ((len && !text) || !n_tokens) return DC_EINVAL;
  if (stride == 0) stride = 1;
  if (!tokens) cap = 0;
  uint32_t n = 0, number = 1;
  uint8_t res = 0, stm = 0;
  size_t i = 0, end = len;
  bool bad = false, done = false, numbered = false;
  // {...} and ";" comments, from their first character; returns the index after
  auto skip_comment = [&](size_t k) {
    const char close = text[k] == '{' ? '}' : '\n';
    while (k < len && text[k] != close) ++k;
    return k < len ? k + 1 : len;
  };
  while (!done && !bad) {
    while (i < len && is_space(text[i])) ++i;
    if (i >= len) break;
    const char ch = text[i];
    if (ch == '{' || ch == ';') {
      i = skip_comment(i);
    } else if (ch == '(') {  // a variation, with the variations and comments inside it
      size_t depth = 0;
      while (i < len) {
        if (text[i] == '{' || text[i] == ';') {
          i = skip_comment(i);
          continue;
        }
        if (text[i] == '(') ++depth;
        if (text[i] == ')' && --depth == 0) {
          ++i;
          break;
        }
        ++i;
      }
    } else if (ch == '$') {
      ++i;
      while (i < len && text[i] >= '0' && text[i] <= '9') ++i;
    } else if (ch == '*') {
      end = ++i;
      done = true;
    } else {
      size_t e = i;  // the word: up to white space or the start of a comment or variation
      while (e < len && !is_space(text[e]) && text[e] != '{' && text[e] != ';' && text[e] != '(' && text[e] != ')') ++e;
      if (e == i) e = i + 1;  // a stray ")"
      const size_t wl = e - i;
      const char* w = text + i;
      const uint8_t r = (wl == 3 && !std::memcmp(w, "1-0", 3))       ? 1
                        : (wl == 3 && !std::memcmp(w, "0-1", 3))     ? 2
                        : (wl == 7 && !std::memcmp(w, "1/2-1/2", 7)) ? DC_PGN_DRAW
                                                                     : 0;
      if (r) {
        res = r;
        end = i = e;
        done = true;
        continue;
      }
      // a move number: digits, then dots ("12." "12..." "12", also glued: "12.e4")
      size_t d = i;
      uint64_t v = 0;
      while (d < e && text[d] >= '0' && text[d] <= '9') {
        v = v * 10 + (uint64_t)(text[d] - '0');
        if (v > 0xFFFFFFFFull) v = 0xFFFFFFFFull;
        ++d;
      }
      size_t dots = 0;
      while (d + dots < e && text[d + dots] == '.') ++dots;
      if (d > i && (dots || d == e)) {
        if (!numbered && n == 0) {  // the first number, if it stands before the first move
          number = (uint32_t)v;
          stm = dots >= 2 ? 1 : 0;
        }
        numbered = true;
        i = d + dots;
        continue;
      }
      uint32_t tok;
      if (!parse_san(w, wl, tok)) {
        end = i;  // the offset of the word
        bad = true;
        break;
      }
      if (n < cap) tokens[(size_t)n * stride] = tok;
      if (n == 0xFFFFFFFFu) {
        end = i;
        bad = true;
        break;
      }
      ++n;
      i = e;
    }
  }
  *n_tokens = n;
  if (result) *result = res;
  if (first_fullmove) *first_fullmove = number;
  if (first_stm) *first_stm = stm;
  if (consumed) *consumed = (done || bad) ? end : len;
  if (bad) return DC_EINVAL;
  return (cap && n > cap) ? DC_EINVAL : DC_SUCCESS;
}

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
