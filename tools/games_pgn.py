#!/usr/bin/env python3
"""Prints seeded games as PGN.

Generates `--games` games of `--plies` plies with dc_gen_games under the
standard rules (seed, noise as dc_gen_games; the generator starts from the
start position), replays them with dc_replay_san from the start position or
from `--fen`, and prints one PGN game each: the Result tag (with SetUp and FEN
when a start FEN is given), then the movetext dc_pgn_movetext makes of the
game's SAN bytes.  A game that ended without a checkmate names its termination
in a comment before the result.  Rejected moves (the generator's junk, or moves
that do not fit `--fen`) are not part of a game and are left out.

With `--own-starts N` every game begins at a position of its own: the one its
first k plies lead to, k seeded per game from 0..N (dc_replay_outcome_starts'
final positions and clocks), written as SetUp and FEN tags; the rest of the game
is replayed from there (dc_replay_san_starts).

    python tools/games_pgn.py --seed 2024 --games 4 --plies 300 --noise 0
    python tools/games_pgn.py --games 3000 --plies 120 --own-starts 40 > starts.pgn
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "distributed-chess_amd"))

import numpy as np  # noqa: E402

import dchess  # noqa: E402

TERMINATION = {dchess.GO_STALEMATE: "stalemate", dchess.GO_DEAD: "dead position (insufficient material)",
               dchess.GO_FIVEFOLD: "fivefold repetition", dchess.GO_SEVENTYFIVE: "seventy-five moves without a "
               "pawn move or capture", dchess.GO_ONGOING: "unfinished"}


def pgn(moves, san, outcome, fen, fullmove, stm):
    """One game's PGN text from its column of moves and SAN bytes."""
    result = int(outcome["result"])
    text = dchess.pgn_movetext(moves, san, result, fullmove, stm)
    body, token = text.rsplit(" ", 1) if " " in text else ("", text)
    tags = [f'[Result "{token}"]']
    if fen:
        tags += ['[SetUp "1"]', f'[FEN "{fen}"]']
    if result in TERMINATION:
        body = (body + " " if body else "") + "{" + TERMINATION[result] + "}"
    return "\n".join(tags) + "\n\n" + (body + " " if body else "") + token + "\n"


def own_starts(eng, moves, seed, most):
    """Cuts every game after a seeded number (0..most) of its own plies.  Returns
    (the remaining plies [n_plies, n_games] padded with MOVE_NONE, the positions at
    the cut, their half-move clocks, full-move numbers)."""
    n_plies, n_games = moves.shape
    cut = np.random.default_rng(seed).integers(0, min(most, n_plies) + 1, n_games)
    ply = np.arange(n_plies)[:, None]
    head = np.where(ply < cut[None, :], moves, dchess.MOVE_NONE).astype(np.uint16)
    out, san, _, _, _, _, finals = eng.replay_san_starts(head, want_bitmap=False, want_digests=False)
    tail = np.full_like(moves, dchess.MOVE_NONE)
    for g in range(n_games):
        tail[:n_plies - cut[g], g] = moves[cut[g]:, g]
    fullmoves = 1 + (san != 0xFF).sum(axis=0) // 2
    return tail, finals, out["halfmove"].astype(np.uint16), fullmoves


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=2024)
    ap.add_argument("--games", type=int, default=4)
    ap.add_argument("--plies", type=int, default=300)
    ap.add_argument("--noise", type=int, default=0, help="junk moves per 256 plies")
    ap.add_argument("--fen", default=None, help="replay from this position instead of the start position")
    ap.add_argument("--own-starts", type=int, default=None, metavar="N",
                    help="begin every game after a seeded number (0..N) of its own plies")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    if a.fen and a.own_starts is not None:
        ap.error("--fen and --own-starts exclude each other")

    eng = dchess.Engine(a.device)
    moves = eng.gen_games(a.seed, 0, a.games, a.plies, a.noise, dchess.RULES_FIDE)
    if a.own_starts is not None:
        moves, starts, halfmoves, fullmoves = own_starts(eng, moves, a.seed, a.own_starts)
        out, san = eng.replay_san_starts(moves, starts, halfmoves, want_bitmap=False, want_digests=False,
                                         want_finals=False)[:2]
        for g in range(a.games):
            fen = dchess.pos_to_fen(starts[g], int(halfmoves[g]), int(fullmoves[g]))
            print(pgn(moves[:, g], san[:, g], out[g], fen, int(fullmoves[g]), int(starts[g]["stm"])))
        eng.close()
        return
    start, halfmove, fullmove, stm, fen = None, 0, 1, 0, None
    if a.fen:
        start = dchess.pos_from_fen(a.fen)
        halfmove, fullmove = dchess.fen_clocks(a.fen)
        stm = int(start["stm"])
        fen = dchess.pos_to_fen(start, halfmove, fullmove)
    out, san, _, _, _, _ = eng.replay_san(moves, start, halfmove, want_bitmap=False, want_digests=False)
    for g in range(a.games):
        print(pgn(moves[:, g], san[:, g], out[g], fen, fullmove, stm))
    eng.close()


if __name__ == "__main__":
    main()
