// tests/cpp/perft_stats_oracle.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The expected values of dc_perft_stats (tests/golden/make_perft_stats.py
// builds and drives this program; the binary is not committed).  Moves come
// from the fastcpu oracle (gen_moves, make); every move that reaches a leaf is
// classified here with a mailbox attack walk from the king's square -- no
// bitboards, no shared code with the kernels.
//
// stdin, one request per line:
//   <rules 0|1> <depth> <stm> <castle> <ep> <64 cells, -1 or colour * 8 + kind>
// stdout, one line per request: n_root, then per root move its move word and
// the 11 counters (DC_PS_* order).
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <string>
#include <thread>
#include <vector>
#include <iostream>

#include "../../oracle/fastcpu.hpp"

using namespace fastcpu;

namespace {

enum { NODES, CAPTURES, EP, CASTLES, PROMOTIONS, CHECKS, DISCOVERED, DOUBLE, CHECKMATES, STALEMATES, KING_CAPTURES,
       COUNT };
struct Row {
  uint64_t c[COUNT] = {};
};

inline bool on_board(int r, int f) { return r >= 0 && r < 8 && f >= 0 && f < 8; }

// The squares of the pieces of colour `by` that attack square s; returns how many.
int attackers(const Pos& p, int s, int by, int out[16]) {
  int n = 0;
  const int r = s >> 3, f = s & 7;
  auto is = [&](int rr, int ff, int kind) {
    return on_board(rr, ff) && p.sq[8 * rr + ff] == by * 8 + kind;
  };
  static const int kn[8][2] = {{1, 2}, {2, 1}, {2, -1}, {1, -2}, {-1, -2}, {-2, -1}, {-2, 1}, {-1, 2}};
  for (auto& d : kn)
    if (is(r + d[0], f + d[1], N)) out[n++] = 8 * (r + d[0]) + f + d[1];
  // a white pawn attacks upward: it stands one row below its target
  const int pr = by == 0 ? r - 1 : r + 1;
  for (int df : {-1, 1})
    if (is(pr, f + df, P)) out[n++] = 8 * pr + f + df;
  for (int dr = -1; dr <= 1; ++dr)
    for (int df = -1; df <= 1; ++df) {
      if (!dr && !df) continue;
      if (is(r + dr, f + df, K)) out[n++] = 8 * (r + dr) + f + df;
      const bool diag = dr && df;
      for (int rr = r + dr, ff = f + df; on_board(rr, ff); rr += dr, ff += df) {
        const int8_t q = p.sq[8 * rr + ff];
        if (q < 0) continue;
        if (q == by * 8 + Q || q == by * 8 + (diag ? B : R)) out[n++] = 8 * rr + ff;
        break;
      }
    }
  return n;
}

void classify(const Pos& par, Rules rules, const Move& m, Row& row) {
  row.c[NODES]++;
  const int8_t mover = par.sq[m.from], victim = par.sq[m.to];
  if (rules == RULES_REF) {
    if (victim >= 0) row.c[CAPTURES]++;
    if (victim >= 0 && (victim & 7) == K) row.c[KING_CAPTURES]++;
    return;
  }
  const bool pawn = (mover & 7) == P, king = (mover & 7) == K;
  const bool ep = pawn && victim < 0 && (m.from & 7) != (m.to & 7);
  const bool castle = king && std::abs((int)m.to - (int)m.from) == 2;
  if (victim >= 0 || ep) row.c[CAPTURES]++;
  if (ep) row.c[EP]++;
  if (castle) row.c[CASTLES]++;
  if (m.promo) row.c[PROMOTIONS]++;
  Pos ch = par;
  make(ch, rules, m);
  int ksq = -1;
  for (int s = 0; s < 64; ++s)
    if (ch.sq[s] == ch.stm * 8 + K) {
      ksq = s;
      break;
    }
  int chk[16];
  const int nchk = ksq >= 0 ? attackers(ch, ksq, 1 - ch.stm, chk) : 0;
  Move buf[256];
  const bool no_moves = gen_moves(ch, rules, buf) == 0;
  if (nchk) {
    row.c[CHECKS]++;
    if (nchk >= 2) {
      row.c[DOUBLE]++;
    } else {
      const int rook_to = (m.from + m.to) / 2;  // the castled rook lands between the king's squares
      if (chk[0] != m.to && !(castle && chk[0] == rook_to)) row.c[DISCOVERED]++;
    }
    if (no_moves) row.c[CHECKMATES]++;
  } else if (no_moves) {
    row.c[STALEMATES]++;
  }
}

void walk(const Pos& p, Rules rules, unsigned depth, Row& row) {
  Move mv[256];
  const int n = gen_moves(p, rules, mv);
  for (int i = 0; i < n; ++i) {
    if (depth == 1) {
      classify(p, rules, mv[i], row);
    } else {
      Pos c = p;
      make(c, rules, mv[i]);
      walk(c, rules, depth - 1, row);
    }
  }
}

}  // namespace

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    int rules, depth, stm, castle, ep;
    in >> rules >> depth >> stm >> castle >> ep;
    Pos p{};
    for (int s = 0; s < 64; ++s) {
      int v;
      in >> v;
      p.sq[s] = (int8_t)v;
    }
    if (!in || depth < 1) {
      std::fprintf(stderr, "bad request: %s\n", line.c_str());
      return 1;
    }
    p.stm = (uint8_t)stm;
    p.castle = (uint8_t)castle;
    p.ep = (int8_t)ep;
    const Rules r = rules ? RULES_FIDE : RULES_REF;
    Move roots[256];
    const int n = gen_moves(p, r, roots);
    std::vector<Row> rows(n);
    std::atomic<int> next{0};
    auto work = [&] {
      for (int i; (i = next.fetch_add(1)) < n;) {
        if (depth == 1) {
          classify(p, r, roots[i], rows[i]);
        } else {
          Pos c = p;
          make(c, r, roots[i]);
          walk(c, r, (unsigned)depth - 1, rows[i]);
        }
      }
    };
    std::vector<std::thread> pool;
    for (int t = 0; t < 8; ++t) pool.emplace_back(work);
    for (auto& t : pool) t.join();
    std::printf("%d", n);
    for (int i = 0; i < n; ++i) {
      std::printf(" %u", (unsigned)encode(roots[i]));
      for (int k = 0; k < COUNT; ++k) std::printf(" %llu", (unsigned long long)rows[i].c[k]);
    }
    std::printf("\n");
    std::fflush(stdout);
  }
  return 0;
}
