"""CPU test: the model of dc_san_resolve (tests/san_resolve_model.py) pinned by
hand on constructed positions, and the round trip SAN text -> token -> move
word over the seeded batches of tests/test_gpu_san.py.

The model is what the GPU tests compare the kernel with, so it is pinned first.
Every FEN, token and expected word is written out here; CASES is what
tests/test_gpu_san_resolve.py batches per start position.

A push and a capture onto one square are never both legal (the push needs the
square empty, the capture needs it occupied, and an en-passant square lies in
front of no pawn of the capturing side), so "e4 is the push even when dxe4 is
legal" is pinned as its two halves: with a black pawn on e4, "e4" finds no match
(it never means dxe4) and "dxe4" is the capture; without it "e4" is the push."""
import numpy as np
import pytest

import oracle_lib as O
import outcome_model as M
import san_model as S
import san_resolve_model as R

mv = M.mv
NOMATCH, AMBIGUOUS, MALFORMED, NONE = R.NOMATCH, R.AMBIGUOUS, R.MALFORMED, R.NONE
CASTLES = "r3k2r/8/8/8/8/8/8/R3K2R w KQkq - 0 1"
THREE_QUEENS = "1k6/8/8/8/4Q2Q/8/8/K6Q w - - 0 1"
TWO_KNIGHTS = "4k3/8/8/8/8/5N2/8/1N2K3 w - - 0 1"
PROMO = "3r1k2/4P3/8/8/8/8/8/4K3 w - - 0 1"

# name, FEN (None = startpos), tokens (SAN text, or a raw token word), the words expected
CASES = [
    # the f3 knight is pinned on the f-file by the f8 rook: only b1 can go to d2
    ("pinned_twin", "5r1k/8/8/8/8/5N2/8/1N3K2 w - - 0 1", ["Nd2"], [mv("b1d2")]),
    # check from the e8 rook; the c3 knight is pinned by the b4 bishop and cannot interpose
    ("twin_cannot_answer_check", "4r1k1/8/8/8/1b6/2N5/8/4K1N1 w - - 0 1", ["Ne2"], [mv("g1e2")]),
    ("push_with_a_d_pawn_beside", "4k3/8/8/8/8/3P4/4P3/4K3 w - - 0 1", ["e4"], [mv("e2e4")]),
    ("single_push", "4k3/8/8/8/8/3P4/4P3/4K3 w - - 0 1", ["e3"], [mv("e2e3")]),
    # a black pawn on e4: "e4" is never dxe4, "dxe4" is
    ("e4_is_never_the_capture", "4k3/8/8/8/4p3/3P4/4P3/4K3 w - - 0 1", ["e4", "dxe4"], [NOMATCH, mv("d3e4")]),
    ("en_passant", "4k3/8/8/3pP3/8/8/8/4K3 w - d6 0 1", ["exd6"], [mv("e5d6")]),
    # taking en passant would clear the fifth rank between the a5 king and the h5 rook
    ("en_passant_rank_pin", "8/8/8/KPp4r/8/8/8/4k3 w - c6 0 1", ["bxc6", "b6"], [NOMATCH, mv("b5b6")]),
    ("promotion", PROMO, ["e8=Q"], [mv("e7e8q")]),
    ("promotion_missing", PROMO, ["e8", "e8=R+"], [NOMATCH, mv("e7e8r")]),
    ("promotion_off_the_last_rank", PROMO, ["e7=Q", "exd8=B"], [NOMATCH, mv("e7d8b")]),
    ("capture_promotion", "4r1k1/3P4/8/8/8/8/8/6K1 w - - 0 1", ["dxe8=N"], [mv("d7e8n")]),
    ("castle_white_short", CASTLES, ["O-O"], [mv("e1g1")]),
    ("castle_white_long", CASTLES, ["O-O-O"], [mv("e1c1")]),
    ("castle_black_short", CASTLES.replace(" w ", " b "), ["O-O"], [mv("e8g8")]),
    ("castle_black_long", CASTLES.replace(" w ", " b "), ["0-0-0"], [mv("e8c8")]),
    # the f8 rook attacks f1
    ("castle_through_attack", "4kr2/8/8/8/8/8/8/R3K2R w KQ - 0 1", ["O-O", "O-O-O"], [NOMATCH, mv("e1c1")]),
    ("king_token_never_castles", CASTLES, ["Kg1", "Kc1", "Kf1"], [NOMATCH, NOMATCH, mv("e1f1")]),
    ("ambiguous_then_resolved", TWO_KNIGHTS, ["Nd2", "Nbd2"], [AMBIGUOUS, mv("b1d2")]),
    ("ambiguous_then_other", TWO_KNIGHTS, ["Nd2", "Nfd2", "Nd2"], [AMBIGUOUS, mv("f3d2"), NOMATCH]),
    ("long_form", None, ["Nhf3", "Ng1f3", "e7e5", "e2e4"], [NOMATCH, mv("g1f3"), mv("e7e5"), mv("e2e4")]),
    ("three_queens", THREE_QUEENS, ["Qh4e1"], [mv("h4e1")]),
    ("three_queens_short_of_hints", THREE_QUEENS, ["Qe1", "Qhe1", "Q4e1", "Q1e1", "Qee1"],
     [AMBIGUOUS, AMBIGUOUS, AMBIGUOUS, mv("h1e1"), NOMATCH]),
    ("after_mate", None, ["f3", "e5", "g4", "Qh4#", "e4", "Nf3", "O-O"],
     [mv("f2f3"), mv("e7e5"), mv("g2g4"), mv("d8h4"), NOMATCH, NOMATCH, NOMATCH]),
    ("none_keeps_the_turn", None, [NONE, "e4", NONE, NONE, "e5", NONE], [0xFFFF, mv("e2e4"), 0xFFFF, 0xFFFF,
                                                                          mv("e7e5"), 0xFFFF]),
    ("malformed_kind", None, [R.token("e4", kind=6), R.token("e4", kind=7), "e4"], [MALFORMED, MALFORMED, mv("e2e4")]),
    ("malformed_promo", PROMO, [R.token("e8", promo=5), R.token("e8", promo=7), "e8=N"],
     [MALFORMED, MALFORMED, mv("e7e8n")]),
    ("malformed_reserved", None, [R.token("e4") | (1 << 25), R.token("e4") | (1 << 31), "e4"],
     [MALFORMED, MALFORMED, mv("e2e4")]),
    ("malformed_both_castles", CASTLES, [R.OO | R.OOO, "O-O"], [MALFORMED, mv("e1g1")]),
    # bits 22-24 ("x", "+", "#") are the parser's record and do not count as fields
    ("malformed_castle_with_fields", CASTLES, [R.OO | R.token("g1"), R.OOO | R.FILE_GIVEN, R.OO | R.X | R.CHECK],
     [MALFORMED, MALFORMED, mv("e1g1")]),
    ("malformed_promo_on_a_piece", PROMO, [R.token("f1", kind=R.K, promo=4), "Kf1"], [MALFORMED, mv("e1f1")]),
]


def tokens_of(items):
    return [t if isinstance(t, int) else R.parse(t) for t in items]


@pytest.mark.parametrize("name,fen,items,want", CASES, ids=[c[0] for c in CASES])
def test_constructed(name, fen, items, want):
    start = O.Pos.from_fen(fen) if fen else None
    words, first_bad, counts = R.walk(tokens_of(items), start)
    assert [hex(w) for w in words] == [hex(w) for w in want]
    flagged = [p for p, w in enumerate(want) if w != 0xFFFF and w & 0x8000]
    assert first_bad == (flagged[0] if flagged else len(items))
    assert counts == [sum(w != 0xFFFF for w in want), sum(not w & 0x8000 for w in want),
                      want.count(NOMATCH), want.count(AMBIGUOUS), want.count(MALFORMED)]


def test_parser_forms():
    assert R.parse("e4") == R.token("e4")
    assert R.parse("Nbd2") == R.token("d2", R.N, file=1)
    assert R.parse("R1a2") == R.token("a2", R.R, rank=0)
    assert R.parse("Qh4xe1#") == R.token("e1", R.Q, file=7, rank=3, x=True, mate=True)
    assert R.parse("exd8=Q+") == R.token("d8", R.P, promo=4, file=4, x=True, check=True)
    assert R.parse("bxc3") == R.token("c3", R.P, file=1, x=True) != R.parse("Bxc3") == R.token("c3", R.B, x=True)
    assert R.parse("O-O") == R.OO == R.parse("0-0") and R.parse("O-O-O+!?") == R.OOO | R.CHECK
    for bad in ("", "e9", "Ne", "Qe8=Q", "e.p.", "e4e", "Pe4", "o-o"):
        with pytest.raises(ValueError):
            R.parse(bad)


def token_classes(tokens):
    """How often each class of token occurs in a batch."""
    t = tokens[tokens != NONE]
    kind, file, rank = (t >> 6) & 7, t & R.FILE_GIVEN != 0, t & R.RANK_GIVEN != 0
    castle = t & (R.OO | R.OOO) != 0
    piece = (kind != R.P) & ~castle
    return {"tokens": int(t.size), "file": int((piece & file & ~rank).sum()), "rank": int((piece & rank & ~file).sum()),
            "promotion": int(((t >> 9) & 7 != 0).sum()), "O-O": int((t & R.OO != 0).sum()),
            "O-O-O": int((t & R.OOO != 0).sum()),
            "pawn_capture": int(((kind == R.P) & ~castle & (t & R.X != 0) & file).sum())}


def en_passants(moves, san):
    """Accepted pawn captures onto an empty square, counted by making the games' moves."""
    n = 0
    for g in range(moves.shape[1]):
        pos = O.Pos()
        for p in np.flatnonzero(san[:, g] != S.NONE):
            m, b = int(moves[p, g]), int(san[p, g])
            if (b & 7) == R.P and b & S.CAPTURE and int(pos.cells[(m >> 6) & 63]) < 0:
                n += 1
            pos = O.fast_make(pos, m, O.FIDE)
    return n


@pytest.mark.parametrize("noise", [0, 32])
def test_round_trip(noise):
    """Every accepted ply of the 257 x 600 seeded batch, written as SAN text by the
    SAN model and read back by this model's parser, resolves to the move that was
    played; no ply is left out."""
    moves, san, tokens = R.seeded(noise)
    ok = san != S.NONE
    assert ((tokens != NONE) == ok).all()
    cl = token_classes(tokens)
    cl["en_passant"] = en_passants(moves, san)
    print(noise, cl)
    for k, v in cl.items():
        assert v >= 1, (k, cl)
    words, first_bad, counts = R.walk_batch(tokens)
    bad = np.argwhere(words != np.where(ok, moves, 0xFFFF))
    assert len(bad) == 0, [(int(p), int(g), hex(int(words[p, g])), hex(int(moves[p, g]))) for p, g in bad[:5]]
    assert (first_bad == moves.shape[0]).all()
    assert counts.tolist() == [int(ok.sum()), int(ok.sum()), 0, 0, 0]


def test_file_and_rank_together():
    """The class the seeded batches need not hold: both hints, from the pinned Qh4e1."""
    tok = R.parse(S.san_text(mv("h4e1"), R.Q | S.FILE | S.RANK))
    assert tok & R.FILE_GIVEN and tok & R.RANK_GIVEN
    assert R.walk([tok], O.Pos.from_fen(THREE_QUEENS))[0] == [mv("h4e1")]
