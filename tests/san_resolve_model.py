"""Plain-Python model of dc_san_resolve -- TEST INFRASTRUCTURE ONLY.

For a position it takes the oracle's legal FIDE move list (oracle_lib's mailbox
engine, as outcome_model.py does) and keeps the moves that fit the token by the
candidate rules of include/dchess.h "notation input": the moved piece's kind,
the origin file and rank where given, a pawn's file (the written one, else the
target's), the promotion field, and castling only through the castle bits.
0, 1 or more fits give the word.  A column of tokens is walked exactly as the
kernel is specified to: a flagged word leaves the position where it was.

It also has its own text -> token parser (a regular expression), so the tests
can build tokens without the product's parser.
"""
import functools
import re

import numpy as np

import oracle_lib as O
import san_model as S

NONE = 0xFFFFFFFF
MOVE_NONE, NOMATCH, AMBIGUOUS, MALFORMED = 0xFFFF, 0x8001, 0x8002, 0x8003
FILE_GIVEN, RANK_GIVEN, OO, OOO, X, CHECK, MATE = 1 << 12, 1 << 16, 1 << 20, 1 << 21, 1 << 22, 1 << 23, 1 << 24
P, N, B, R, Q, K = range(6)

_SAN = re.compile(r"^([KQRBN])?([a-h])?([1-8])?(x)?([a-h])([1-8])(?:=([QRBN]))?([+#])?[!?]*$")
_CASTLE = re.compile(r"^[O0]-[O0](-[O0])?([+#])?[!?]*$")


def token(target=0, kind=P, promo=0, file=None, rank=None, x=False, check=False, mate=False):
    """A token word from its fields (target: a square index or a name like 'd2')."""
    t = target if isinstance(target, int) else 8 * (int(target[1]) - 1) + (ord(target[0]) - ord("a"))
    tok = t | (kind << 6) | (promo << 9)
    if file is not None:
        tok |= FILE_GIVEN | (file << 13)
    if rank is not None:
        tok |= RANK_GIVEN | (rank << 17)
    return tok | (X if x else 0) | (CHECK if check else 0) | (MATE if mate else 0)


def parse(text):
    """SAN text -> token word; ValueError where it is no SAN token."""
    m = _CASTLE.match(text)
    if m:
        return (OOO if m.group(1) else OO) | {None: 0, "+": CHECK, "#": MATE}[m.group(2)]
    m = _SAN.match(text)
    if not m:
        raise ValueError(text)
    piece, f, r, x, tf, tr, promo, suffix = m.groups()
    if promo and piece:
        raise ValueError(text)
    return token(tf + tr, "PNBRQK".index(piece) if piece else P, " NBRQ".index(promo) if promo else 0,
                 "abcdefgh".index(f) if f else None, int(r) - 1 if r else None, bool(x), suffix == "+",
                 suffix == "#")


def malformed(tok):
    kind, promo, castle = (tok >> 6) & 7, (tok >> 9) & 7, (tok >> 20) & 3
    return bool(tok >> 25) or kind > 5 or promo > 4 or castle == 3 or bool(castle and tok & 0xFFFFF) or \
        bool(kind != P and promo)


def fits(pos, legal, tok):
    """The legal moves of pos that the (well-formed) token can mean."""
    us = pos.stm
    castle = (tok >> 20) & 3
    if castle:
        kings = [s for s in range(64) if int(pos.cells[s]) == us * 8 + K]
        if len(kings) != 1:
            return []
        k = kings[0]
        y = (k & 7) + (2 if castle & 1 else -2)
        if not 0 <= y < 8:
            return []
        return [m for m in legal if (m & 63) == k and ((m >> 6) & 63) == (k & ~7) + y]
    t, kind, promo = tok & 63, (tok >> 6) & 7, (tok >> 9) & 7
    file = (tok >> 13) & 7 if tok & FILE_GIVEN else None
    rank = (tok >> 17) & 7 if tok & RANK_GIVEN else None
    if kind == P and file is None:
        file = t & 7  # "e4" is the e-pawn's push, whatever may capture there
    out = []
    for m in legal:
        f, to, pr = m & 63, (m >> 6) & 63, (m >> 12) & 7
        if to != t or int(pos.cells[f]) != us * 8 + kind or pr != promo:
            continue
        if kind == K and abs((f & 7) - (to & 7)) == 2:
            continue  # castling is written O-O / O-O-O only
        if file is not None and (f & 7) != file:
            continue
        if rank is not None and (f >> 3) != rank:
            continue
        out.append(m)
    return out


def resolve(pos, tok, legal=None):
    """The word of one token in one position."""
    if malformed(tok):
        return MALFORMED
    if legal is None:
        legal = [int(m) for m in O.fast_gen_moves(pos, O.FIDE)]
    ms = fits(pos, legal, tok)
    return NOMATCH if not ms else AMBIGUOUS if len(ms) > 1 else ms[0]


def walk(tokens, start=None):
    """One game's column of tokens.  Returns (words, first_bad, counts[5])."""
    pos = start.copy() if start is not None else O.Pos()
    legal = None
    words, first_bad, counts = [], len(tokens), [0] * 5
    for ply, tok in enumerate(tokens):
        tok = int(tok)
        if tok == NONE:
            words.append(MOVE_NONE)
            continue
        if legal is None:
            legal = [int(m) for m in O.fast_gen_moves(pos, O.FIDE)]
        w = resolve(pos, tok, legal)
        words.append(w)
        counts[0] += 1
        if w & 0x8000:
            counts[{NOMATCH: 2, AMBIGUOUS: 3, MALFORMED: 4}[w]] += 1
            first_bad = min(first_bad, ply)
        else:
            counts[1] += 1
            pos, legal = O.fast_make(pos, w, O.FIDE), None
    return words, first_bad, counts


def walk_batch(tokens, start=None):
    """tokens: uint32 [n_plies, n_games].  Returns (moves uint16 [n_plies, n_games],
    first_bad uint32 [n_games], counts uint64 [5])."""
    tokens = np.ascontiguousarray(tokens, np.uint32)
    n_plies, n_games = tokens.shape
    moves = np.zeros((n_plies, n_games), np.uint16)
    first_bad = np.zeros(n_games, np.uint32)
    counts = np.zeros(5, np.uint64)
    for g in range(n_games):
        w, fb, c = walk(tokens[:, g], start)
        moves[:, g] = w
        first_bad[g] = fb
        counts += np.array(c, np.uint64)
    return moves, first_bad, counts


def pad_tokens(columns):
    """Token lists of unequal length -> uint32 [n_plies, n_games], padded with NONE."""
    n = max(len(c) for c in columns)
    out = np.full((n, len(columns)), NONE, np.uint32)
    for g, c in enumerate(columns):
        out[:len(c), g] = c
    return out


@functools.lru_cache(maxsize=None)
def seeded(noise):
    """The 257-game batch of tests/test_gpu_san.py for one noise level, annotated
    once a process: (moves, SAN bytes, tokens built from san_model.san_text through
    parse() with NONE where the byte is 0xFF)."""
    mv = O.fast_gen_games(2024, 0, 257, 600, noise, O.FIDE)
    san, _ = S.annotate_batch(mv)
    tokens = np.full(mv.shape, NONE, np.uint32)
    for p, g in np.argwhere(san != S.NONE):
        tokens[p, g] = parse(S.san_text(int(mv[p, g]), int(san[p, g])))
    for a in (mv, san, tokens):
        a.setflags(write=False)
    return mv, san, tokens
