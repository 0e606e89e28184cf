#!/usr/bin/env python3
"""Replays a PGN file on the GPU.

Splits FILE into games (dchess.pgn_games), parses each game's movetext into
SAN tokens (dc_pgn_parse_movetext), batches the games that share a start
position (the FEN tag through dc_pos_from_fen / dc_fen_clocks, else the start
position; columns padded with SAN_TOKEN_NONE), resolves the tokens to move
words (dc_san_resolve) and replays those under the standard rules
(dc_replay_san).  Prints the histogram of adjudicated outcomes, the games in
which a token did not resolve (with the token's number and why), the games
whose movetext is not SAN, and the games whose adjudicated result contradicts
their Result tag.  A game the board does not decide (a resignation, an agreed
draw, an unfinished game) contradicts nothing.

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
    """Resolves and replays the games, one batch per start position.  Returns
    {index: (moves u16 [n_tokens], first_bad, outcome record)}."""
    groups = {}
    for g in games:
        groups.setdefault(g[1].get("FEN"), []).append(g)
    done = {}
    for fen, members in groups.items():
        start, halfmove = None, 0
        if fen is not None:
            start = dchess.pos_from_fen(fen)
            halfmove = min(dchess.fen_clocks(fen)[0], 150)
        n_plies = max(max(len(m[2]) for m in members), 1)
        tokens = np.full((n_plies, len(members)), dchess.SAN_TOKEN_NONE, np.uint32)
        for k, m in enumerate(members):
            tokens[:len(m[2]), k] = m[2]
        moves, first_bad, _ = eng.resolve_san(tokens, start)
        out = eng.replay_san(moves, start, halfmove, want_bitmap=False, want_digests=False)[0]
        for k, m in enumerate(members):
            done[m[0]] = (moves[:len(m[2]), k].copy(), int(first_bad[k]), out[k])
    return done


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("file")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    with open(a.file, encoding="utf-8") as f:
        games, broken = load(f.read())
    eng = dchess.Engine(a.device)
    done = replay(eng, games) if games else {}
    eng.close()

    print(f"{len(games) + len(broken)} games, {len(games)} parsed, {len(broken)} not")
    hist = np.zeros(dchess.GO_COUNT, np.int64)
    for _, _, out in done.values():
        hist[int(out["result"])] += 1
    for k, name in enumerate(dchess.GO_NAMES):
        print(f"  {name:12s} {int(hist[k])}")
    for i, msg in broken:
        print(f"game {i + 1}: {msg}")
    unresolved = contradicted = 0
    for i, tags, tokens, tag in games:
        moves, first_bad, out = done[i]
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
    return 1 if broken or unresolved or contradicted else 0


if __name__ == "__main__":
    sys.exit(main())
