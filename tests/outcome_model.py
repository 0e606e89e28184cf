"""Plain-Python model of dc_replay_outcome -- TEST INFRASTRUCTURE ONLY.

The legal moves and the made positions come from the oracle's independent
mailbox engine (oracle_lib.fast_gen_moves / fast_make under FIDE); everything
the adjudication adds is written here, in Python, on the oracle's cell board:
its own attack walk for "in check", the dead-position rule, the en-passant
filter of FIDE 9.2.2, the half-move clock and a Counter of positions that is
cleared whenever the clock restarts.
"""
from collections import Counter

import numpy as np

import oracle_lib as O

ONGOING, WHITE_WINS, BLACK_WINS, STALEMATE, DEAD, FIVEFOLD, SEVENTYFIVE = range(7)
P, N, B, R, Q, K = range(6)

_KNIGHT = ((1, 2), (2, 1), (2, -1), (1, -2), (-1, -2), (-2, -1), (-2, 1), (-1, 2))
_ORTH = ((1, 0), (-1, 0), (0, 1), (0, -1))
_DIAG = ((1, 1), (1, -1), (-1, 1), (-1, -1))


def sq(name):
    """'e4' -> square index 8 * row + column (row 0 = White's back rank)."""
    return 8 * (int(name[1]) - 1) + (ord(name[0]) - ord("a"))


def mv(text):
    """'e2e4' / 'e7e8q' -> move word from | to << 6 | promo << 12."""
    promo = " nbrq".index(text[4]) if len(text) > 4 else 0
    return sq(text[0:2]) | (sq(text[2:4]) << 6) | (promo << 12)


def line(text):
    return [mv(t) for t in text.split()]


def in_check(pos):
    """Is the side to move's king attacked?  An attack walk from the king."""
    c = pos.cells
    us = pos.stm
    king = [s for s in range(64) if c[s] == us * 8 + K]
    if not king:
        return False
    kx, ky = divmod(king[0], 8)

    def at(x, y):
        return int(c[8 * x + y]) if 0 <= x < 8 and 0 <= y < 8 else None

    def enemy(v, kinds):
        return v is not None and v >= 0 and (v >> 3) != us and (v & 7) in kinds

    # an enemy pawn attacks towards our side: White's pawns go up the rows
    px = kx + 1 if us == 0 else kx - 1
    if enemy(at(px, ky - 1), (P,)) or enemy(at(px, ky + 1), (P,)):
        return True
    if any(enemy(at(kx + dx, ky + dy), (N,)) for dx, dy in _KNIGHT):
        return True
    if any(enemy(at(kx + dx, ky + dy), (K,)) for dx, dy in _ORTH + _DIAG):
        return True
    for dirs, kinds in ((_ORTH, (R, Q)), (_DIAG, (B, Q))):
        for dx, dy in dirs:
            x, y = kx + dx, ky + dy
            while (v := at(x, y)) is not None:
                if v >= 0:
                    if enemy(v, kinds):
                        return True
                    break
                x, y = x + dx, y + dy
    return False


def dead(pos):
    """Insufficient material (DC_ST_DEAD): only kings, knights and bishops, and at
    most one knight or bishop in all, or no knight and all bishops on one colour."""
    knights, bishops = 0, []
    for s in range(64):
        v = int(pos.cells[s])
        if v < 0:
            continue
        k = v & 7
        if k == K:
            continue
        if k == N:
            knights += 1
        elif k == B:
            bishops.append(((s >> 3) + (s & 7)) & 1)
        else:
            return False
    return knights + len(bishops) <= 1 or (knights == 0 and len(set(bishops)) <= 1)


def ep_usable(pos, legal):
    """FIDE 9.2.2: a legal pawn move onto the en-passant square from another file."""
    if pos.ep < 0:
        return False
    for m in legal:
        f, t = m & 63, (m >> 6) & 63
        if t == pos.ep and (f & 7) != (t & 7) and int(pos.cells[f]) == pos.stm * 8 + P:
            return True
    return False


def adjudicate(moves, start=None, start_halfmove=0):
    """One game.  moves: move words (0xFFFF skipped).  Returns a dict: result,
    end_ply, repeats, halfmove, accept (one bool per ply), validated, accepted
    and pos (the final position)."""
    pos = start.copy() if start is not None else O.Pos()
    clock = int(start_halfmove)
    seen = Counter()
    n_plies = len(moves)
    accept = [False] * n_plies
    validated = accepted = 0

    def judge():
        legal = [int(m) for m in O.fast_gen_moves(pos, O.FIDE)]
        key = (pos.cells.tobytes(), pos.stm, pos.castle, pos.ep if ep_usable(pos, legal) else -1)
        seen[key] += 1
        rep = seen[key]
        if not legal:
            res = (WHITE_WINS if pos.stm else BLACK_WINS) if in_check(pos) else STALEMATE
        elif dead(pos):
            res = DEAD
        elif rep >= 5:
            res = FIVEFOLD
        elif clock >= 150:
            res = SEVENTYFIVE
        else:
            res = ONGOING
        return res, rep, set(legal)

    result, repeats, legal = judge()
    end_ply = 0 if result != ONGOING else n_plies
    for ply in range(n_plies):
        if result != ONGOING:
            break
        m = int(moves[ply])
        if m == 0xFFFF:
            continue
        validated += 1
        if m not in legal:
            continue
        accepted += 1
        accept[ply] = True
        f, t = m & 63, (m >> 6) & 63
        reset = (int(pos.cells[f]) & 7) == P or int(pos.cells[t]) >= 0
        pos = O.fast_make(pos, m, O.FIDE)
        if reset:
            clock = 0
            seen.clear()
        else:
            clock += 1
        result, repeats, legal = judge()
        if result != ONGOING:
            end_ply = ply + 1
    return {"result": result, "end_ply": end_ply, "repeats": repeats, "halfmove": clock, "accept": accept,
            "validated": validated, "accepted": accepted, "pos": pos}


def adjudicate_batch(moves, start=None, start_halfmove=0):
    """moves: uint16 [n_plies, n_games] ply-major.  Returns (outcomes as a list of
    (result, end_ply, repeats, halfmove), bitmap u64 [n_plies, words], counts[7],
    stats dict (validated, accepted, rejected), digests u64 [n_games])."""
    moves = np.ascontiguousarray(moves, np.uint16)
    n_plies, n_games = moves.shape
    words = (n_games + 63) // 64
    bitmap = np.zeros((n_plies, words), np.uint64)
    counts = [0] * 7
    out, digests = [], np.zeros(n_games, np.uint64)
    val = acc = 0
    for g in range(n_games):
        r = adjudicate(moves[:, g], start, start_halfmove)
        out.append((r["result"], r["end_ply"], r["repeats"], r["halfmove"]))
        counts[r["result"]] += 1
        val += r["validated"]
        acc += r["accepted"]
        digests[g] = O.digest(r["pos"].cells, r["pos"].stm)
        for ply, ok in enumerate(r["accept"]):
            if ok:
                bitmap[ply, g >> 6] |= np.uint64(1 << (g & 63))
    return out, bitmap, counts, {"validated": val, "accepted": acc, "rejected": val - acc}, digests
