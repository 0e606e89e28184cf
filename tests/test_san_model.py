"""CPU test: the SAN model (tests/san_model.py) against strings pinned by hand.

The model is what the GPU tests compare dc_replay_san with, so it is pinned
first: the standard examples of each SAN form, the disambiguation cases in
which a pin or a check decides which pieces count (FIDE C.10.3 counts only
pieces that can legally make the move), and the games of test_outcome_model.py
as full movetext with their result token."""
import pytest

import oracle_lib as O
import outcome_model as M
import san_model as S
from test_outcome_model import PINNED

# FEN (None = startpos), moves, the SAN tokens of the moves
LINES = [
    (None, "f2f3 e7e5 g2g4 d8h4", "f3 e5 g4 Qh4#"),
    (None, "e2e4 e7e5 d1h5 b8c6 f1c4 g8f6 h5f7", "e4 e5 Qh5 Nc6 Bc4 Nf6 Qxf7#"),
    (None, "g1f3 d7d5 d2d4 g8f6 b1d2", "Nf3 d5 d4 Nf6 Nbd2"),
    ("4k3/8/8/8/R7/8/8/R3K3 w - - 0 1", "a1a2", "R1a2"),
    ("4k3/8/8/8/R7/8/8/R3K3 w - - 0 1", "a4a2", "R4a2"),
    ("1k6/8/8/8/4Q2Q/8/8/K6Q w - - 0 1", "h4e1", "Qh4e1"),
    # the c3 knight is pinned by the b4 bishop and does not count
    ("4k3/8/8/8/1b6/2N5/8/4K1N1 w - - 0 1", "g1e2", "Ne2"),
    ("3r1k2/4P3/8/8/8/8/8/4K3 w - - 0 1", "e7d8q", "exd8=Q+"),
    ("4k3/8/8/3pP3/8/8/8/4K3 w - d6 0 1", "e5d6", "exd6"),
    ("5k2/8/8/8/8/8/8/4K2R w K - 0 1", "e1g1", "O-O+"),
    ("3k4/8/8/8/8/8/8/R3K3 w Q - 0 1", "e1c1", "O-O-O+"),
    # the e2 rook is pinned by the e8 rook but may move along the e-file: it counts, both ways
    ("4r2k/8/8/8/R7/8/4R3/4K3 w - - 0 1", "a4e4", "Rae4"),
    ("4r2k/8/8/8/R7/8/4R3/4K3 w - - 0 1", "e2e4", "Ree4"),
    # ... and does not when the target is off its pin line (only the a-rook reaches a2 legally)
    ("4r2k/8/8/8/R7/8/4R3/4K3 w - - 0 1", "a4a2", "Ra2"),
    # White is in check from the f3 knight; the e2 queen attacks f3 too, but it is pinned by
    # the e8 rook (on other moves it could still slide along the e-file): only the h5 queen
    # can take, no origin is written
    ("1k2r3/8/8/7Q/8/5n2/4Q3/4K3 w - - 0 1", "h5f3", "Qxf3"),
    # the same knights as above with a rook check on the e-file: the pinned one cannot interpose
    ("4r1k1/8/8/8/1b6/2N5/8/4K1N1 w - - 0 1", "g1e2", "Ne2"),
    # discovered check: the knight leaves the e-file, the e1 rook gives the check
    ("4k3/8/8/8/4N3/8/8/K3R3 w - - 0 1", "e4c5", "Nc5+"),
    # double check: rook and knight
    ("4k3/8/8/8/4N3/8/8/K3R3 w - - 0 1", "e4d6", "Nd6+"),
    # a file alone tells three knights apart only if no other stands on it: b1 and b5 share the b-file
    ("4k3/8/8/1N6/8/8/8/1N2K1N1 w - - 0 1", "b1c3", "N1c3"),
    ("4k3/8/8/1N6/8/8/8/1N2K3 w - - 0 1", "b5c3", "N5c3"),
    # captures by pieces, with and without an origin
    ("4k3/8/8/3p4/8/2N1N3/8/4K3 w - - 0 1", "c3d5", "Ncxd5"),
    # a black promotion with capture and check, lower-case promo letter in, upper-case out
    ("4k3/8/8/8/8/8/1p6/R2K4 b - - 0 1", "b2a1n", "bxa1=N"),
    ("4k3/8/8/8/8/8/1p6/2RK4 b - - 0 1", "b2c1q", "bxc1=Q+"),
    ("4k3/8/8/8/8/8/p7/4K3 b - - 0 1", "a2a1r", "a1=R+"),
]


@pytest.mark.parametrize("fen,moves,want", LINES, ids=[f"{i}_{l[2].split()[-1]}" for i, l in enumerate(LINES)])
def test_pinned_san(fen, moves, want):
    start = O.Pos.from_fen(fen) if fen else None
    toks, _ = S.game_text(M.line(moves), start)
    assert " ".join(toks) == want


def test_double_check_bytes():
    """The check and mate bits come from the child position, whoever gives the check."""
    pos = O.Pos.from_fen("4k3/8/8/8/4N3/8/8/K3R3 w - - 0 1")
    for text, flags in (("e4c5", S.CHECK), ("e4d6", S.CHECK), ("e4g5", S.CHECK), ("a1b1", 0), ("e1d1", 0)):
        r = S.annotate(M.line(text), pos)
        assert r["san"][0] & (S.CHECK | S.MATE) == flags, text
    r = S.annotate(M.line("f2f3 e7e5 g2g4 d8h4"))
    assert [b & (S.CHECK | S.MATE) for b in r["san"]] == [0, 0, 0, S.CHECK | S.MATE]
    assert [b & 7 for b in r["san"]] == [M.P, M.P, M.P, M.Q]


def test_rejected_and_post_end_plies_have_no_byte():
    r = S.annotate(M.line("e2e5 f2f3 e7e5 g2g4 d8h4 a2a3") + [0xFFFF])
    assert [b == S.NONE for b in r["san"]] == [True, False, False, False, False, True, True]
    assert r["end_ply"] == 5


def test_black_to_move_start():
    start = O.Pos.from_fen("rnbqkbnr/pppppppp/8/8/4P3/8/PPPP1PPP/RNBQKBNR b KQkq e3 0 1")
    toks, text = S.game_text(M.line("e7e5 g1f3 b8c6"), start)
    assert toks == ["e5", "Nf3", "Nc6"]
    assert text == "1... e5 2. Nf3 Nc6 *"
    _, text = S.game_text(M.line("e7e5 g1f3 b8c6"), start, first_fullmove=7)
    assert text == "7... e5 8. Nf3 Nc6 *"
    _, text = S.game_text(M.line("e7e5"), start)
    assert text == "1... e5 *"


def _cycle(first, n, a, b, c, d):
    """n rounds of "N. a b N+1. c d" starting at move number `first`."""
    return " ".join(f"{first + 2 * i}. {a} {b} {first + 2 * i + 1}. {c} {d}" for i in range(n))


MOVETEXT = {
    "fools_mate_plus_one": "1. f3 e5 2. g4 Qh4# 0-1",
    "loyd_stalemate": ("1. e3 a5 2. Qh5 Ra6 3. Qxa5 h5 4. h4 Rah6 5. Qxc7 f6 6. Qxd7+ Kf7 7. Qxb7 Qd3 8. Qxb8 Qh7 "
                       "9. Qxc8 Kg6 10. Qe6 1/2-1/2"),
    "fivefold_startpos": _cycle(1, 4, "Nf3", "Nf6", "Ng1", "Ng8") + " 1/2-1/2",
    "fivefold_dead_ep": "1. e4 Nf6 " + _cycle(2, 3, "Nf3", "Ng8", "Ng1", "Nf6") + " 8. Nf3 Ng8 9. Ng1 1/2-1/2",
    "fivefold_live_ep": "1... d5 " + _cycle(2, 4, "Kd1", "Kd8", "Ke1", "Ke8") + " 10. Kd1 1/2-1/2",
    "fivefold_pinned_ep": "1. d4 Ka5 " + _cycle(2, 3, "Ke1", "Ka4", "Kd1", "Ka5") + " 8. Ke1 Ka4 9. Kd1 1/2-1/2",
    "seventyfive_148": "1. Nf3 Nf6 1/2-1/2",
    "seventyfive_at_start": "1/2-1/2",
    "fifty_is_a_claim": "1. Nf3 Nf6 2. Ng1 *",
    "dead_after_capture": "1. Rh8+ Kf7 2. Rh7+ Kg8 3. Rg7+ Kxg7 1/2-1/2",
    "illegal_first_move": "1. f3 e5 2. g4 Qh4# 0-1",
}


@pytest.mark.parametrize("name,fen,halfmove,moves,want", PINNED, ids=[p[0] for p in PINNED])
def test_pinned_games_as_movetext(name, fen, halfmove, moves, want):
    start = O.Pos.from_fen(fen) if fen else None
    _, text = S.game_text(M.line(moves), start, halfmove)
    assert text == MOVETEXT[name]


def test_formatter_forms():
    mv = M.mv
    assert S.san_text(mv("e2e4"), M.P) == "e4"
    assert S.san_text(mv("e4d5"), M.P | S.CAPTURE) == "exd5"
    assert S.san_text(mv("g1f3"), M.N | S.FILE | S.RANK | S.CAPTURE | S.CHECK) == "Ng1xf3+"
    assert S.san_text(mv("e8g8"), M.K | S.CHECK | S.MATE) == "O-O#"
    assert S.san_text(mv("e8c8"), M.K) == "O-O-O"
    assert S.san_text(mv("e1f1"), M.K) == "Kf1"
    assert S.san_text(mv("a7a8b"), M.P | S.CHECK) == "a8=B+"
    assert S.movetext([], [], M.ONGOING) == "*"
    assert S.movetext([mv("e2e4"), 0xFFFF, mv("e7e5")], [M.P, S.NONE, M.P], M.DEAD) == "1. e4 e5 1/2-1/2"
