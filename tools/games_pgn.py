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

    python tools/games_pgn.py --seed 2024 --games 4 --plies 300 --noise 0
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "distributed-chess_amd"))

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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=2024)
    ap.add_argument("--games", type=int, default=4)
    ap.add_argument("--plies", type=int, default=300)
    ap.add_argument("--noise", type=int, default=0, help="junk moves per 256 plies")
    ap.add_argument("--fen", default=None, help="replay from this position instead of the start position")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()

    eng = dchess.Engine(a.device)
    moves = eng.gen_games(a.seed, 0, a.games, a.plies, a.noise, dchess.RULES_FIDE)
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
