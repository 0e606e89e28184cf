#!/usr/bin/env python3
"""Replays a PGN file on the GPU.

Splits FILE into games (dchess.pgn_games), parses each game's movetext into
SAN tokens (dc_pgn_parse_movetext), puts all games into one batch, each with
its own start position and half-move clock (the FEN tag through
dc_pos_from_fen / dc_fen_clocks, else the start position; columns padded with
SAN_TOKEN_NONE), resolves the tokens to move words (dc_san_resolve_starts) and
replays those under the standard rules (dc_replay_san_starts): two calls a
file, whatever its FEN tags.  Prints the histogram of adjudicated outcomes, the games in
which a token did not resolve (with the token's number and why), the games
whose movetext is not SAN, and the games whose adjudicated result contradicts
their Result tag.  A game the board does not decide (a resignation, an agreed
draw, an unfinished game) contradicts nothing.  With --final-fen, also the FEN
of the position every game stopped in.

    python tools/games_pgn.py --games 100 --plies 400 > games.pgn
    python tools/pgn_replay.py games.pgn
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "distributed-chess_amd"))

import dchess  # noqa: E402

RESULT_TOKEN = {dchess.GO_ONGOING: "*", dchess.GO_WHITE_WINS: "1-0", dchess.GO_BLACK_WINS: "0-1"}
PARSED_TOKEN = ("*", "1-0", "0-1", "1/2-1/2")
FLAG_NAMES = {dchess.MOVE_NOMATCH: "no legal move fits", dchess.MOVE_AMBIGUOUS: "more than one legal move fits",
              dchess.MOVE_MALFORMED: "malformed token"}


def load(text):
    """[(index, tags, tokens, result token)] of the games that parse, [(index, message)] of the others."""
    games, broken = [], []
    for i, (tags, movetext) in enumerate(dchess.pgn_games(text)):
        try:
            tokens, result, _, _, _ = dchess.pgn_parse_movetext(movetext)
        except dchess.DChessError as e:
            at = getattr(e, "offset", 0)  # a byte offset into the utf-8 text
            word = movetext.encode()[at:at + 12].decode(errors="replace")
            broken.append((i, f"no SAN token at byte {at} of the movetext: {word!r}"))
            continue
        games.append((i, tags, tokens, tags.get("Result", PARSED_TOKEN[result])))
    return games, broken


def replay(eng, games):
    """Resolves and replays the games in one batch, every game from its own start
    (one resolve_san_starts call and one replay_san_starts call, whatever the FEN tags).
    Returns {index: (moves u16 [n_tokens], first_bad, outcome record, final FEN)}."""
    n = len(games)
    starts = np.array([dchess.startpos()] * n, dchess.POS_DTYPE)
    halfmoves, fullmoves = np.zeros(n, np.uint16), [1] * n
    for k, g in enumerate(games):
        fen = g[1].get("FEN")
        if fen is not None:
            starts[k] = dchess.pos_from_fen(fen)
            halfmove, fullmoves[k] = dchess.fen_clocks(fen)
            halfmoves[k] = min(halfmove, 150)
    # columns ordered by side to move: a wave that holds both sides runs both sides'
    # rule code one after the other; the results are keyed by game
    order = np.argsort(starts["stm"], kind="stable")
    games = [games[k] for k in order]
    starts, halfmoves, fullmoves = starts[order], halfmoves[order], [fullmoves[k] for k in order]
    n_plies = max(max(len(g[2]) for g in games), 1)
    tokens = np.full((n_plies, n), dchess.SAN_TOKEN_NONE, np.uint32)
    for k, g in enumerate(games):
        tokens[:len(g[2]), k] = g[2]
    moves, first_bad, _, _ = eng.resolve_san_starts(tokens, starts, want_finals=False)
    out, san, _, _, _, _, finals = eng.replay_san_starts(moves, starts, halfmoves, want_bitmap=False,
                                                         want_digests=False)
    done = {}
    played = (san != 0xFF).sum(axis=0)
    for k, g in enumerate(games):
        # Black's move completes a full move
        fullmove = fullmoves[k] + (int(starts[k]["stm"]) + int(played[k])) // 2
        fen = dchess.pos_to_fen(finals[k], int(out[k]["halfmove"]), fullmove)
        done[g[0]] = (moves[:len(g[2]), k].copy(), int(first_bad[k]), out[k], fen)
    return done


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("file")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--final-fen", action="store_true", help="print the FEN of the position every game stopped in")
    a = ap.parse_args()
    with open(a.file, encoding="utf-8") as f:
        games, broken = load(f.read())
    eng = dchess.Engine(a.device)
    done = replay(eng, games) if games else {}
    eng.close()

    print(f"{len(games) + len(broken)} games, {len(games)} parsed, {len(broken)} not")
    hist = np.zeros(dchess.GO_COUNT, np.int64)
    for _, _, out, _ in done.values():
        hist[int(out["result"])] += 1
    for k, name in enumerate(dchess.GO_NAMES):
        print(f"  {name:12s} {int(hist[k])}")
    for i, msg in broken:
        print(f"game {i + 1}: {msg}")
    unresolved = contradicted = 0
    for i, tags, tokens, tag in games:
        moves, first_bad, out, _ = done[i]
        if first_bad < len(tokens):
            unresolved += 1
            print(f"game {i + 1}: move {first_bad + 1} of {len(tokens)} did not resolve "
                  f"({FLAG_NAMES.get(int(moves[first_bad]), hex(int(moves[first_bad])))})")
        result = int(out["result"])
        if result != dchess.GO_ONGOING and RESULT_TOKEN.get(result, "1/2-1/2") != tag:
            contradicted += 1
            print(f"game {i + 1}: Result \"{tag}\" but the board says {dchess.GO_NAMES[result]} "
                  f"after {int(out['end_ply'])} of {len(tokens)} moves")
    print(f"{unresolved} games with an unresolved move, {contradicted} with a contradicted result")
    if a.final_fen:
        for i, _, _, _ in games:
            print(f"game {i + 1}: {done[i][3]}")
    return 1 if broken or unresolved or contradicted else 0


if __name__ == "__main__":
    sys.exit(main())
