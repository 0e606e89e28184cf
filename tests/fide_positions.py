"""Constructed FIDE positions, their classifier and three plain-Python models
-- TEST INFRASTRUCTURE ONLY.

Seeded playouts from the start position almost never reach the positions in
which a bitboard move generator goes wrong: a legal en-passant capture, one
that is geometrically there but illegal, double checks, several pins, castling
through attacked squares.  `constructed(n, seed)` builds such positions from
motifs; `features(pos)` says which classes a position belongs to, so a test can
assert its coverage before it trusts a comparison.

Everything here is a mailbox walk over the oracle's cell board
(cells[8 * rank + file] = -1 or colour * 8 + kind, kinds P N B R Q K = 0..5)
and shares no code with oracle/fastcpu.cpp or the kernels:

  py_legal_moves(pos)   pseudo-legal moves, make, "is my king attacked"
  stats_row(pos, move)  the eleven DC_PS_* counters of one move, from the
                        definitions in include/dchess.h
  features(pos)         the coverage classes
"""
import functools

import numpy as np

import oracle_lib as O

P, N, B, R, Q, K = range(6)
KNIGHT = ((1, 2), (2, 1), (2, -1), (1, -2), (-1, -2), (-2, -1), (-2, 1), (-1, 2))
ORTH = ((1, 0), (-1, 0), (0, 1), (0, -1))
DIAG = ((1, 1), (1, -1), (-1, 1), (-1, -1))
ALL8 = ORTH + DIAG
PS_NODES, PS_CAPTURES, PS_EP, PS_CASTLES, PS_PROMOTIONS, PS_CHECKS, PS_DISCOVERED, PS_DOUBLE, PS_CHECKMATES, \
    PS_STALEMATES, PS_KING_CAPTURES = range(11)
PS_COUNT = 11

# FEN, legal moves of the side to move (both engines and, for the first five,
# tests/golden/perft_stats.json agree), what it is here for
HAND = [
    ("8/8/8/R2pP2k/8/8/8/4K3 w - d6 0 1", 17, "an en-passant capture that discovers a check along the rank"),
    ("5k2/8/8/8/8/8/8/4K2R w K - 0 1", 15, "a castle that checks"),
    ("4k3/P7/8/8/8/8/8/4K3 w - - 0 1", 9, "a promotion that checks"),
    ("4k3/8/4N3/8/8/8/8/4RK2 w - - 0 1", 20, "knight moves that discover the rook, double checks"),
    ("7k/5Q2/8/8/8/8/8/K7 w - - 0 1", 26, "stalemating moves"),
    ("8/k7/8/8/7Q/8/8/K3Q2Q w - - 0 1", 51, "three queens reach e4: Qh1e4 needs file and rank"),
    ("8/8/8/8/k2Pp2Q/8/8/3K4 b - d3 0 1", 6, "en passant would expose the king along the rank"),
    ("8/8/8/2k5/3Pp3/8/8/4K3 b - d3 0 1", 9, "the pushed pawn checks: capturing it en passant is an evasion"),
    ("7k/5Q2/6K1/8/8/8/8/8 b - - 0 1", 0, "stalemate"),
]


# ------------------------------------------------------------ mailbox basics
def _on(r, f):
    return 0 <= r < 8 and 0 <= f < 8


def checkers(cells, s, by):
    """The squares from which a piece of colour `by` attacks square s."""
    out = []
    r0, f0 = s >> 3, s & 7
    pr = r0 - 1 if by == 0 else r0 + 1  # a white pawn attacks upwards, so it stands one rank below
    if 0 <= pr < 8:
        for f in (f0 - 1, f0 + 1):
            if 0 <= f < 8 and cells[8 * pr + f] == by * 8 + P:
                out.append(8 * pr + f)
    for dr, df in KNIGHT:
        r, f = r0 + dr, f0 + df
        if _on(r, f) and cells[8 * r + f] == by * 8 + N:
            out.append(8 * r + f)
    for dr, df in ALL8:
        r, f = r0 + dr, f0 + df
        if _on(r, f) and cells[8 * r + f] == by * 8 + K:
            out.append(8 * r + f)
    for dirs, slider in ((ORTH, by * 8 + R), (DIAG, by * 8 + B)):
        for dr, df in dirs:
            r, f = r0 + dr, f0 + df
            while _on(r, f):
                c = cells[8 * r + f]
                if c >= 0:
                    if c == slider or c == by * 8 + Q:
                        out.append(8 * r + f)
                    break
                r, f = r + dr, f + df
    return out


def attacked(cells, s, by):
    return bool(checkers(cells, s, by))


def king_square(cells, color):
    for s in range(64):
        if cells[s] == color * 8 + K:
            return s
    return -1


def _state(pos):
    return [int(c) for c in pos.cells], pos.stm, pos.castle, pos.ep


def in_check(pos):
    cells, stm, _, _ = _state(pos)
    ks = king_square(cells, stm)
    return ks >= 0 and attacked(cells, ks, 1 - stm)


def _reach(cells, s):
    """Squares the piece on s reaches by its ordinary move or capture (no pawn
    pushes onto pieces, no en passant, no castling): empty or enemy squares."""
    pc = cells[s]
    color, kind = pc >> 3, pc & 7
    r0, f0 = s >> 3, s & 7
    out = []
    if kind == P:
        d = 1 if color == 0 else -1
        r1 = r0 + d
        if 0 <= r1 < 8:
            if cells[8 * r1 + f0] < 0:
                out.append(8 * r1 + f0)
                if r0 == (1 if color == 0 else 6) and cells[8 * (r1 + d) + f0] < 0:
                    out.append(8 * (r1 + d) + f0)
            for f in (f0 - 1, f0 + 1):
                if 0 <= f < 8 and cells[8 * r1 + f] >= 0 and (cells[8 * r1 + f] >> 3) != color:
                    out.append(8 * r1 + f)
        return out
    if kind in (N, K):
        for dr, df in (KNIGHT if kind == N else ALL8):
            r, f = r0 + dr, f0 + df
            if _on(r, f) and (cells[8 * r + f] < 0 or (cells[8 * r + f] >> 3) != color):
                out.append(8 * r + f)
        return out
    for dr, df in {B: DIAG, R: ORTH, Q: ALL8}.get(kind, ()):
        r, f = r0 + dr, f0 + df
        while _on(r, f):
            c = cells[8 * r + f]
            if c < 0:
                out.append(8 * r + f)
            else:
                if (c >> 3) != color:
                    out.append(8 * r + f)
                break
            r, f = r + dr, f + df
    return out


def _pseudo(cells, stm, castle, ep):
    """Pseudo-legal (from, to, promo) of the side to move, lazily; castling
    already has its own conditions checked except the king's arrival square."""
    last = 7 if stm == 0 else 0
    for s in range(64):
        pc = cells[s]
        if pc < 0 or (pc >> 3) != stm:
            continue
        kind = pc & 7
        for t in _reach(cells, s):
            if kind == P and (t >> 3) == last:
                for promo in (1, 2, 3, 4):
                    yield s, t, promo
            else:
                yield s, t, 0
        if kind == P and ep >= 0:
            d = 1 if stm == 0 else -1
            if (ep >> 3) == (s >> 3) + d and abs((ep & 7) - (s & 7)) == 1:
                yield s, ep, 0
        if kind == K and s == (4 if stm == 0 else 60):
            them = 1 - stm
            rook = stm * 8 + R
            kside, qside = (1, 2) if stm == 0 else (4, 8)
            if castle & (kside | qside) and not attacked(cells, s, them):
                if castle & kside and cells[s + 3] == rook and cells[s + 1] < 0 and cells[s + 2] < 0 \
                        and not attacked(cells, s + 1, them):
                    yield s, s + 2, 0
                if castle & qside and cells[s - 4] == rook and cells[s - 1] < 0 and cells[s - 2] < 0 \
                        and cells[s - 3] < 0 and not attacked(cells, s - 1, them):
                    yield s, s - 2, 0


_RIGHTS = {4: 3, 0: 2, 7: 1, 60: 12, 56: 8, 63: 4}  # a move from or to the square loses these rights


def _make(cells, stm, castle, ep, f, t, promo):
    """FIDE articles 3.1-3.8 on a copy of the board."""
    c = list(cells)
    pc = c[f]
    kind = pc & 7
    c[t], c[f] = pc, -1
    if kind == P:
        if t == ep and (f & 7) != (t & 7):
            c[(f & ~7) | (t & 7)] = -1  # the pawn that just passed stands beside the capturer
        if promo:
            c[t] = stm * 8 + promo
    if kind == K and abs(t - f) == 2 and (t >> 3) == (f >> 3):
        if t > f:
            c[f + 1], c[f + 3] = c[f + 3], -1
        else:
            c[f - 1], c[f - 4] = c[f - 4], -1
    castle &= ~(_RIGHTS.get(f, 0) | _RIGHTS.get(t, 0))
    new_ep = (f + t) // 2 if kind == P and abs(t - f) == 16 else -1
    return c, 1 - stm, castle, new_ep


def _legal(cells, stm, castle, ep):
    out = []
    for f, t, promo in _pseudo(cells, stm, castle, ep):
        c = _make(cells, stm, castle, ep, f, t, promo)[0]
        ks = king_square(c, stm)
        if ks < 0 or not attacked(c, ks, 1 - stm):
            out.append(f | (t << 6) | (promo << 12))
    return out


def _has_legal(cells, stm, castle, ep):
    for f, t, promo in _pseudo(cells, stm, castle, ep):
        c = _make(cells, stm, castle, ep, f, t, promo)[0]
        ks = king_square(c, stm)
        if ks < 0 or not attacked(c, ks, 1 - stm):
            return True
    return False


def py_legal_moves(pos):
    """The legal move words of pos in (from, to, promo) order."""
    return sorted(_legal(*_state(pos)), key=lambda m: (m & 63, (m >> 6) & 63, m >> 12))


def py_make(pos, move):
    c, stm, castle, ep = _make(*_state(pos), move & 63, (move >> 6) & 63, (move >> 12) & 7)
    return O.Pos(np.array(c, np.int8), stm, castle, ep)


# --------------------------------------------------------- perft statistics
def _stats_row(state, move):
    cells, stm, castle, ep = state
    f, t, promo = move & 63, (move >> 6) & 63, (move >> 12) & 7
    kind = cells[f] & 7
    row = [0] * PS_COUNT
    row[PS_NODES] = 1
    is_ep = kind == P and t == ep and (f & 7) != (t & 7)
    is_castle = kind == K and abs((t & 7) - (f & 7)) == 2
    row[PS_CAPTURES] = int(cells[t] >= 0 or is_ep)
    row[PS_EP] = int(is_ep)
    row[PS_CASTLES] = int(is_castle)
    row[PS_PROMOTIONS] = int(promo != 0)
    child = _make(cells, stm, castle, ep, f, t, promo)
    ks = king_square(child[0], 1 - stm)
    chk = checkers(child[0], ks, stm) if ks >= 0 else []
    if chk:
        row[PS_CHECKS] = 1
        if len(chk) >= 2:
            row[PS_DOUBLE] = 1
        else:
            rook_to = (f + t) // 2 if is_castle else -1
            if chk[0] != t and chk[0] != rook_to:
                row[PS_DISCOVERED] = 1
    if not _has_legal(*child):
        row[PS_CHECKMATES if chk else PS_STALEMATES] = 1
    return row


def stats_row(pos, move):
    """The eleven DC_PS_* counters of the legal move `move` in pos."""
    return _stats_row(_state(pos), int(move))


def stats_rows(pos, moves):
    st = _state(pos)
    return [_stats_row(st, int(m)) for m in moves]


# ---------------------------------------------------------------- classifier
def _pinned(cells, stm):
    """Own pieces that stand alone between their king and an enemy slider of the line's kind."""
    ks = king_square(cells, stm)
    out = []
    r0, f0 = ks >> 3, ks & 7
    for dirs, slider in ((ORTH, R), (DIAG, B)):
        for dr, df in dirs:
            r, f = r0 + dr, f0 + df
            own = -1
            while _on(r, f):
                c = cells[8 * r + f]
                if c >= 0:
                    if own < 0:
                        if (c >> 3) != stm:
                            break
                        own = 8 * r + f
                    else:
                        if (c >> 3) != stm and (c & 7) in (slider, Q):
                            out.append(own)
                        break
                r, f = r + dr, f + df
    return out


def twin_illegal(pos, legal):
    """Legal N/B/R/Q moves for which another own piece of the same kind reaches
    the target geometrically but not legally."""
    cells, stm, _, _ = _state(pos)
    legal = set(int(m) for m in legal)
    n = 0
    for m in legal:
        f, t = m & 63, (m >> 6) & 63
        if (cells[f] & 7) not in (N, B, R, Q):
            continue
        for s in range(64):
            if s != f and cells[s] == cells[f] and t in _reach(cells, s) and (s | (t << 6)) not in legal:
                n += 1
                break
    return n


def features(pos, legal):
    """The coverage classes of pos; legal = the oracle's legal move words (used
    for membership only)."""
    cells, stm, castle, ep = _state(pos)
    legal = set(int(m) for m in legal)
    ks = king_square(cells, stm)
    chk = checkers(cells, ks, 1 - stm)
    pins = _pinned(cells, stm)
    d = 1 if stm == 0 else -1
    ep_ok = ep_bad = 0
    if ep >= 0:
        for f in ((ep & 7) - 1, (ep & 7) + 1):
            s = 8 * ((ep >> 3) - d) + f
            if 0 <= f < 8 and cells[s] == stm * 8 + P:
                if (s | (ep << 6)) in legal:
                    ep_ok += 1
                else:
                    ep_bad += 1
    home = 4 if stm == 0 else 60
    held = (castle >> (2 * stm)) & 3
    can = [(home | ((home + 2) << 6)) in legal and cells[home] == stm * 8 + K,
           (home | ((home - 2) << 6)) in legal and cells[home] == stm * 8 + K]
    at_home = [cells[home] == stm * 8 + K and cells[home + 3] == stm * 8 + R,
               cells[home] == stm * 8 + K and cells[home - 4] == stm * 8 + R]
    promo = [m for m in legal if m >> 12]
    return {
        "ep_legal": ep_ok >= 1, "ep_two": ep_ok == 2, "ep_illegal": ep_bad >= 1, "ep_in_check": ep_ok >= 1 and bool(chk),
        "double_check": len(chk) >= 2, "single_check": len(chk) == 1, "pins2": len(pins) >= 2, "pins1": len(pins) == 1,
        "castle_legal": any(can),
        "castle_denied": any(held >> i & 1 and at_home[i] and not can[i] for i in (0, 1)),
        "stale_right": any(held >> i & 1 and not at_home[i] for i in (0, 1)),
        "promotion": bool(promo), "promotion_capture": any((m & 7) != ((m >> 6) & 7) for m in promo),
        "no_moves": not legal,
    }


def consistent(pos):
    """One king a side and not adjacent, no pawn on a back rank, the side not to
    move not in check, ep -1 or behind an enemy pawn that can just have pushed."""
    cells, stm, castle, ep = _state(pos)
    for color in (0, 1):
        if sum(c == color * 8 + K for c in cells) != 1:
            return False
    a, b = king_square(cells, 0), king_square(cells, 1)
    if max(abs((a >> 3) - (b >> 3)), abs((a & 7) - (b & 7))) <= 1:
        return False
    if any(c >= 0 and (c & 7) == P for c in cells[:8] + cells[56:]):
        return False
    if attacked(cells, king_square(cells, 1 - stm), stm):
        return False
    if ep >= 0:
        d = 1 if stm == 0 else -1  # the enemy pawn came towards us
        if (ep >> 3) != (5 if stm == 0 else 2):
            return False
        if cells[ep - 8 * d] != (1 - stm) * 8 + P or cells[ep] >= 0 or cells[ep + 8 * d] >= 0:
            return False
    return not (castle & ~15)


# ----------------------------------------------------------------- generator
_MIX = [P] * 8 + [N] * 2 + [B] * 2 + [R] * 3 + [Q] * 2


class _Board:
    def __init__(self, rng, stm):
        self.rng, self.us, self.them = rng, stm, 1 - stm
        self.cells = [-1] * 64
        self.castle, self.ep = 0, -1
        self.keep = set()  # squares that have to stay empty

    def put(self, r, f, color, kind):
        if not _on(r, f):
            return False
        s = 8 * r + f
        if self.cells[s] >= 0 or s in self.keep or (kind == P and r in (0, 7)):
            return False
        if kind == K:
            o = king_square(self.cells, 1 - color)
            if o >= 0 and max(abs((o >> 3) - r), abs((o & 7) - f)) <= 1:
                return False
        self.cells[s] = color * 8 + kind
        return True

    def ri(self, lo, hi):
        return int(self.rng.integers(lo, hi))

    def chance(self, p):
        return float(self.rng.random()) < p

    def kind(self):
        return _MIX[self.ri(0, len(_MIX))]


def _ep_pair(b, mode):
    """An enemy pawn on its fourth rank with ep behind it; own pawns beside it."""
    us, them = b.us, b.them
    d = 1 if us == 0 else -1
    r = 4 if us == 0 else 3      # the enemy pawn's rank (its fourth), the capturers' too
    f = b.ri(0, 8)
    b.put(r, f, them, P)
    b.ep = 8 * (r + d) + f
    b.keep |= {b.ep, 8 * (r + 2 * d) + f}
    side = [-1, 1][b.ri(0, 2)]
    if not _on(r, f + side):
        side = -side
    if mode == "rank":
        # king, own pawn, enemy pawn, enemy rook or queen on one rank (in either order of the pawns)
        b.put(r, f + side, us, P)
        lo, hi = min(f, f + side), max(f, f + side)
        left = [x for x in range(0, lo)]
        right = [x for x in range(hi + 1, 8)]
        if left and right:
            kf, sf = left[b.ri(0, len(left))], right[b.ri(0, len(right))]
            if b.chance(0.5):
                kf, sf = sf, kf
            if b.put(r, kf, us, K):
                b.put(r, sf, them, [R, Q][b.ri(0, 2)])
                for x in range(min(kf, sf) + 1, max(kf, sf)):
                    b.keep.add(8 * r + x)
        return
    b.put(r, f + side, us, P)
    if b.chance(0.6):
        b.put(r, f - side, us, P)
    if mode == "diag":
        # king and an enemy bishop or queen on a diagonal through the pawn that would be captured
        dr, df = DIAG[b.ri(0, 4)]
        a, c = b.ri(1, 4), b.ri(1, 4)
        if _on(r + a * dr, f + a * df) and _on(r - c * dr, f - c * df) and b.put(r + a * dr, f + a * df, us, K):
            b.put(r - c * dr, f - c * df, them, [B, Q][b.ri(0, 2)])
            for i in range(-c + 1, a):
                if i:
                    b.keep.add(8 * (r + i * dr) + f + i * df)
    elif mode == "pawn_check":
        # the pawn that just pushed attacks the king
        b.put(r - d, f + [-1, 1][b.ri(0, 2)], us, K) or b.put(r - d, f - 1, us, K) or b.put(r - d, f + 1, us, K)
    elif mode == "line_check":
        # a slider checks along a rank or diagonal through the ep square: capturing there blocks
        dr, df = (ORTH[2:] + DIAG)[b.ri(0, 6)]
        er = r + d
        a, c = b.ri(1, 3), b.ri(1, 4)
        if _on(er + a * dr, f + a * df) and _on(er - c * dr, f - c * df) and b.put(er + a * dr, f + a * df, us, K):
            b.put(er - c * dr, f - c * df, them, [R if dr == 0 else B, Q][b.ri(0, 2)])
            for i in range(-c + 1, a):
                b.keep.add(8 * (er + i * dr) + f + i * df)


def _kings(b):
    for color in (b.us, b.them):
        if king_square(b.cells, color) >= 0:
            continue
        home = 0 if color == 0 else 7
        if b.chance(0.55) and b.put(home, 4, color, K):
            for rf, right in ((7, 1), (0, 2)):
                if b.chance(0.85) and b.put(home, rf, color, R) and b.chance(0.9):
                    b.castle |= right << (2 * color)
            continue
        while not b.put(b.ri(0, 8), b.ri(0, 8), color, K):
            pass


def _king_line(b):
    ks = king_square(b.cells, b.us)
    dr, df = ALL8[b.ri(0, 8)]
    a, c = b.ri(1, 4), b.ri(1, 4)
    r, f = (ks >> 3) + a * dr, (ks & 7) + a * df
    r2, f2 = r + c * dr, f + c * df
    if not _on(r2, f2) or any(b.cells[8 * ((ks >> 3) + i * dr) + (ks & 7) + i * df] >= 0 for i in range(1, a + c + 1)):
        return False
    match = R if (dr == 0 or df == 0) else B
    enemy = [match, Q][b.ri(0, 2)] if b.chance(0.75) else [k for k in (N, B, R, P) if k != match][b.ri(0, 3)]
    if not b.put(r2, f2, b.them, enemy):
        return False
    if b.chance(0.8):
        b.put(r, f, b.us, b.kind())
    return True


def _battery(b):
    """An own slider behind an own piece on a line of the ENEMY king: the front
    piece's moves discover a check, and some of them check as well."""
    ks = king_square(b.cells, b.them)
    dr, df = ALL8[b.ri(0, 8)]
    a, c = b.ri(1, 4), b.ri(1, 4)
    r, f = (ks >> 3) + a * dr, (ks & 7) + a * df
    if not _on(r + c * dr, f + c * df) or any(b.cells[8 * ((ks >> 3) + i * dr) + (ks & 7) + i * df] >= 0
                                              for i in range(1, a + c + 1)):
        return
    match = R if (dr == 0 or df == 0) else B
    front = [N, N, B, R, P][b.ri(0, 5)]
    if front != match and b.put(r, f, b.us, front):
        b.put(r + c * dr, f + c * df, b.us, [match, Q][b.ri(0, 2)])


def _twins(b):
    """Two or three own pieces of one kind that reach a common square; the first
    one sometimes stands pinned on a line of its king."""
    kind = [N, B, R, Q][b.ri(0, 4)]
    ks = king_square(b.cells, b.us)
    first = -1
    if b.chance(0.6):
        dr, df = ALL8[b.ri(0, 8)]
        a, c = b.ri(1, 3), b.ri(1, 4)
        r, f = (ks >> 3) + a * dr, (ks & 7) + a * df
        match = R if (dr == 0 or df == 0) else B
        if _on(r + c * dr, f + c * df) and all(b.cells[8 * ((ks >> 3) + i * dr) + (ks & 7) + i * df] < 0
                                               for i in range(1, a + c + 1)):
            if b.put(r, f, b.us, kind) and b.put(r + c * dr, f + c * df, b.them, [match, Q][b.ri(0, 2)]):
                first = 8 * r + f
    if first < 0:
        r, f = b.ri(0, 8), b.ri(0, 8)
        if not b.put(r, f, b.us, kind):
            return
        first = 8 * r + f
    reach = [t for t in _reach(b.cells, first)]
    if not reach:
        return
    t = reach[b.ri(0, len(reach))]
    # the squares from which a piece of the kind reaches t: put a twin on t's own reach
    saved = b.cells[t]
    b.cells[t] = b.us * 8 + kind
    back = [s for s in _reach(b.cells, t) if b.cells[s] < 0]
    b.cells[t] = saved
    for _ in range(b.ri(1, 3)):
        if back:
            s = back.pop(b.ri(0, len(back)))
            b.put(s >> 3, s & 7, b.us, kind)


def _boxed_king(b, color):
    """Heavy enemy pieces near a king on the edge: mates, stalemates, no legal move."""
    ks = king_square(b.cells, color)
    r0, f0 = ks >> 3, ks & 7
    for _ in range(b.ri(2, 4)):
        dr, df = b.ri(-2, 3), b.ri(-2, 3)
        b.put(r0 + dr, f0 + df, 1 - color, [R, Q, Q, N][b.ri(0, 4)])


def _one(rng):
    b = _Board(rng, int(rng.integers(0, 2)))
    u = float(rng.random())
    mode = None
    for name, p in (("plain", 0.16), ("pawn_check", 0.07), ("line_check", 0.07), ("rank", 0.06), ("diag", 0.06)):
        if u < p:
            mode = name
            break
        u -= p
    if mode:
        _ep_pair(b, mode)
    edge = b.chance(0.15)
    boxed = b.us if b.chance(0.4) else b.them
    if edge and king_square(b.cells, boxed) < 0:
        b.put([0, 7][b.ri(0, 2)], [0, 7, b.ri(0, 8)][b.ri(0, 3)], boxed, K)
    _kings(b)
    if edge:
        _boxed_king(b, boxed)
    want, tries = b.ri(0, 4), 0
    while want and tries < 12:  # a line that runs off the board or into a piece is drawn again
        want -= _king_line(b)
        tries += 1
    if b.chance(0.2):
        _battery(b)
    if b.chance(0.3):
        _twins(b)
    if b.chance(0.12):  # a pawn about to promote, often with something to capture
        r = 6 if b.us == 0 else 1
        f = b.ri(0, 8)
        if b.put(r, f, b.us, P) and b.chance(0.6):
            b.put(r + (1 if b.us == 0 else -1), f + [-1, 1][b.ri(0, 2)], b.them, [N, B, R, Q][b.ri(0, 4)])
    lone = edge and b.chance(0.6)  # a boxed king without an army: stalemates
    for _ in range(b.ri(1, 5 if lone else 14)):
        b.put(b.ri(0, 8), b.ri(0, 8), 1 - boxed if lone else b.ri(0, 2), b.kind())
    if b.chance(0.1):
        b.castle = b.ri(0, 16)  # stale rights: whatever stands on the home squares
    return O.Pos(np.array(b.cells, np.int8), b.us, b.castle, b.ep)


def constructed(n, seed):
    """n consistent constructed positions, deterministic in (n, seed)."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        p = _one(rng)
        if consistent(p):
            out.append(p)
    return out


def hand_positions():
    return [O.Pos.from_fen(fen) for fen, _, _ in HAND]


SEED, N_CONSTRUCTED = 2025, 640


@functools.lru_cache(maxsize=None)
def position_set():
    """The committed set: constructed(640, SEED) followed by the hand-made positions."""
    return tuple(constructed(N_CONSTRUCTED, SEED) + hand_positions())


def stats_below(pos, depth):
    """stats_row over the leaves of a depth-`depth` tree whose plies above the
    last are the oracle's (fast_gen_moves / fast_make).  Returns (totals,
    {root move: row})."""
    def walk(p, d):
        legal = O.fast_gen_moves(p, O.FIDE)
        if d == 1:
            return [sum(col) for col in zip(*stats_rows(p, legal))] if len(legal) else [0] * PS_COUNT
        acc = [0] * PS_COUNT
        for m in legal:
            acc = [a + b for a, b in zip(acc, walk(O.fast_make(p, int(m), O.FIDE), d - 1))]
        return acc

    roots = O.fast_gen_moves(pos, O.FIDE)
    if depth == 1:
        rows = dict(zip((int(m) for m in roots), stats_rows(pos, roots)))
    else:
        rows = {int(m): walk(O.fast_make(pos, int(m), O.FIDE), depth - 1) for m in roots}
    totals = [sum(col) for col in zip(*rows.values())] if rows else [0] * PS_COUNT
    return totals, rows


def slider_on_king_line(pos):
    """Does an enemy rook or queen stand on the rank or file of the side to
    move's king, or an enemy bishop or queen on one of its diagonals, whatever
    stands between?  Waves in which no lane has one skip that line's scans."""
    cells, stm, _, _ = _state(pos)
    ks = king_square(cells, stm)
    for s in range(64):
        c = cells[s]
        if c < 0 or (c >> 3) == stm or s == ks:
            continue
        dr, df = (s >> 3) - (ks >> 3), (s & 7) - (ks & 7)
        if (c & 7) in (R, Q) and (dr == 0 or df == 0):
            return True
        if (c & 7) in (B, Q) and abs(dr) == abs(df):
            return True
    return False


def verdict_table(pos, legal, promos=(0, 1, 2, 3, 4)):
    """Expected verdicts of the unflagged words from | to << 6 | promo << 12, as
    uint8 [len(promos), 4096], in the order of oracle/fastcpu.cpp::validate: no
    piece on `from`, then a piece of the side not to move, then membership in
    the legal list.  (A flagged word, bit 15, is OOR before all of these.)"""
    cells = np.asarray(pos.cells, np.int64)
    per_from = np.where(cells < 0, O.NO_PIECE, np.where((cells >> 3) != pos.stm, O.WRONG_TURN, O.ILLEGAL))
    base = per_from[np.arange(4096) & 63].astype(np.uint8)
    out = np.repeat(base[None, :], len(promos), axis=0)
    legal = np.asarray(legal, np.int64)
    for i, pr in enumerate(promos):
        out[i, legal[(legal >> 12) == pr] & 4095] = O.OK
    return out
