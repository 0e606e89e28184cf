"""Plain-Python model of dc_replay_san and of the SAN / PGN formatter -- TEST
INFRASTRUCTURE ONLY.

It wraps outcome_model.adjudicate, so a game stops where the adjudication
stops.  The legal moves and the made positions come from the oracle's mailbox
engine (oracle_lib.fast_gen_moves / fast_make under FIDE), "in check" from
outcome_model.in_check.  Disambiguation is done the slow, obvious way: list the
legal moves with the same target made by a piece of the same kind, and look at
the files and ranks they come from (FIDE C.10.3).  The byte, the SAN string and
the movetext are all written here; nothing calls the product's formatter.
"""
import numpy as np

import oracle_lib as O
import outcome_model as M

CAPTURE, FILE, RANK, CHECK, MATE = 0x08, 0x10, 0x20, 0x40, 0x80
NONE = 0xFF
LETTERS = "PNBRQK"
RESULT_TOKEN = {M.ONGOING: "*", M.WHITE_WINS: "1-0", M.BLACK_WINS: "0-1", M.STALEMATE: "1/2-1/2", M.DEAD: "1/2-1/2",
                M.FIVEFOLD: "1/2-1/2", M.SEVENTYFIVE: "1/2-1/2"}


def square_name(s):
    return "abcdefgh"[s & 7] + "12345678"[s >> 3]


def san_byte(pos, legal, m, child, child_legal):
    """The SAN byte of the legal move m in pos (legal: pos's legal moves), child
    being the position it leads to and child_legal that position's legal moves."""
    f, t = m & 63, (m >> 6) & 63
    piece = int(pos.cells[f])
    kind = piece & 7
    byte = kind
    if int(pos.cells[t]) >= 0 or (kind == M.P and (f & 7) != (t & 7)):  # a pawn leaving its file captures
        byte |= CAPTURE
    if kind in (M.N, M.B, M.R, M.Q):
        others = {o & 63 for o in legal if ((o >> 6) & 63) == t and (o & 63) != f and int(pos.cells[o & 63]) == piece}
        if others:
            if not any((o & 7) == (f & 7) for o in others):
                byte |= FILE
            elif not any((o >> 3) == (f >> 3) for o in others):
                byte |= RANK
            else:
                byte |= FILE | RANK
    if M.in_check(child):
        byte |= CHECK
        if not child_legal:
            byte |= MATE
    return byte


def san_text(m, byte):
    """The SAN token of move word m with SAN byte `byte`."""
    f, t, promo = m & 63, (m >> 6) & 63, (m >> 12) & 7
    kind = byte & 7
    if kind == M.K and (t >> 3) == (f >> 3) and abs((t & 7) - (f & 7)) == 2:
        s = "O-O" if t > f else "O-O-O"
    else:
        if kind == M.P:
            s = "abcdefgh"[f & 7] if byte & CAPTURE else ""
        else:
            s = LETTERS[kind]
            if byte & FILE:
                s += "abcdefgh"[f & 7]
            if byte & RANK:
                s += "12345678"[f >> 3]
        if byte & CAPTURE:
            s += "x"
        s += square_name(t)
        if promo:
            s += "=" + " NBRQ"[promo]
    if byte & MATE:
        s += "#"
    elif byte & CHECK:
        s += "+"
    return s


def movetext(moves, san, result, first_fullmove=1, first_stm=0):
    """PGN movetext of one game: plies whose byte is NONE are skipped."""
    out = []
    number, stm, first = int(first_fullmove), int(first_stm), True
    for m, b in zip(moves, san):
        if int(b) == NONE:
            continue
        if stm == 0:
            out.append(f"{number}.")
        elif first:
            out.append(f"{number}...")
        out.append(san_text(int(m), int(b)))
        number += stm
        stm ^= 1
        first = False
    out.append(RESULT_TOKEN[result])
    return " ".join(out)


def annotate(moves, start=None, start_halfmove=0):
    """One game.  outcome_model.adjudicate's dict plus "san": one byte per ply
    (NONE for a rejected, padded or post-end ply)."""
    r = M.adjudicate(moves, start, start_halfmove)
    pos = start.copy() if start is not None else O.Pos()
    legal = None
    san = [NONE] * len(moves)
    for ply, ok in enumerate(r["accept"]):
        if not ok:
            continue
        m = int(moves[ply])
        if legal is None:
            legal = [int(x) for x in O.fast_gen_moves(pos, O.FIDE)]
        assert m in legal
        child = O.fast_make(pos, m, O.FIDE)
        child_legal = [int(x) for x in O.fast_gen_moves(child, O.FIDE)]
        san[ply] = san_byte(pos, legal, m, child, child_legal)
        pos, legal = child, child_legal
    r["san"] = san
    return r


def annotate_batch(moves, start=None, start_halfmove=0):
    """moves: uint16 [n_plies, n_games].  Returns (san uint8 [n_plies, n_games],
    [(result, end_ply)] per game)."""
    moves = np.ascontiguousarray(moves, np.uint16)
    n_plies, n_games = moves.shape
    san = np.full((n_plies, n_games), NONE, np.uint8)
    ends = []
    for g in range(n_games):
        r = annotate(moves[:, g], start, start_halfmove)
        san[:, g] = r["san"]
        ends.append((r["result"], r["end_ply"]))
    return san, ends


def game_text(moves, start=None, start_halfmove=0, first_fullmove=1):
    """(list of SAN tokens of the accepted plies, movetext) of one game given as move words."""
    r = annotate(moves, start, start_halfmove)
    toks = [san_text(int(m), b) for m, b in zip(moves, r["san"]) if b != NONE]
    stm = start.stm if start is not None else 0
    return toks, movetext(moves, r["san"], r["result"], first_fullmove, stm)
