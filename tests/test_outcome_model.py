"""CPU test: the adjudication model (tests/outcome_model.py) on known games.

Each game is pinned as (result, end_ply, repeats, halfmove).  The en-passant
rows are the point of FIDE 9.2.2: fide_make sets the en-passant square after
every double push, so a model (or kernel) comparing the raw square ends the
`e2e4` game one ply late (18), and one ignoring the square ends the `d7d5` game
one ply early (17)."""
import pytest

import oracle_lib as O
import outcome_model as M

SHUFFLE_W = "g1f3 g8f6 f3g1 f6g8"
LOYD = ("e2e3 a7a5 d1h5 a8a6 h5a5 h7h5 h2h4 a6h6 a5c7 f7f6 c7d7 e8f7 d7b7 d8d3 b7b8 d3h7 b8c8 f7g6 c8e6")

# name, FEN (None = startpos), start_halfmove, moves, (result, end_ply, repeats, halfmove)
PINNED = [
    ("fools_mate_plus_one", None, 0, "f2f3 e7e5 g2g4 d8h4 a2a3", (M.BLACK_WINS, 4, 1, 1)),
    ("loyd_stalemate", None, 0, LOYD, (M.STALEMATE, 19, 1, 2)),
    ("fivefold_startpos", None, 0, " ".join([SHUFFLE_W] * 5), (M.FIVEFOLD, 16, 5, 16)),
    ("fivefold_dead_ep", None, 0, "e2e4 " + " ".join(["g8f6 g1f3 f6g8 f3g1"] * 6), (M.FIVEFOLD, 17, 5, 16)),
    ("fivefold_live_ep", "4k3/3p4/8/4P3/8/8/8/4K3 b - - 0 1", 0,
     "d7d5 " + " ".join(["e1d1 e8d8 d1e1 d8e8"] * 6), (M.FIVEFOLD, 18, 5, 17)),
    ("fivefold_pinned_ep", "8/8/8/8/k3p2Q/8/3P4/3K4 w - - 0 1", 0,
     "d2d4 " + " ".join(["a4a5 d1e1 a5a4 e1d1"] * 6), (M.FIVEFOLD, 17, 5, 16)),
    ("seventyfive_148", None, 148, "g1f3 g8f6 f3g1", (M.SEVENTYFIVE, 2, 1, 150)),
    ("seventyfive_at_start", None, 150, "", (M.SEVENTYFIVE, 0, 1, 150)),
    ("fifty_is_a_claim", None, 98, "g1f3 g8f6 f3g1", (M.ONGOING, 3, 1, 101)),
    ("dead_after_capture", "4k3/8/8/8/8/8/8/4K2R w - - 0 1", 0, "h1h8 e8f7 h8h7 f7g8 h7g7 g8g7 e1e2",
     (M.DEAD, 6, 1, 0)),
    ("illegal_first_move", None, 0, "e2e5 f2f3 e7e5 g2g4 d8h4", (M.BLACK_WINS, 5, 1, 1)),
]


def run(fen, halfmove, moves):
    start = O.Pos.from_fen(fen) if fen else None
    r = M.adjudicate(M.line(moves), start, halfmove)
    return r["result"], r["end_ply"], r["repeats"], r["halfmove"]


@pytest.mark.parametrize("name,fen,halfmove,moves,want", PINNED, ids=[p[0] for p in PINNED])
def test_pinned_game(name, fen, halfmove, moves, want):
    assert run(fen, halfmove, moves) == want


def test_rejected_move_leaves_clock_and_counts():
    # the illegal e2e5 is validated and rejected, nothing else changes
    r = M.adjudicate(M.line("e2e5 g1f3"))
    assert (r["validated"], r["accepted"], r["halfmove"], r["repeats"]) == (2, 1, 1, 1)
    assert r["accept"] == [False, True]


def test_moves_after_the_end_are_not_counted():
    r = M.adjudicate(M.line("f2f3 e7e5 g2g4 d8h4 a2a3 a7a6"))
    assert (r["validated"], r["accepted"], r["accept"][4:]) == (4, 4, [False, False])


def test_ep_filter_cases():
    live = O.fast_make(O.Pos.from_fen("4k3/3p4/8/4P3/8/8/8/4K3 b - - 0 1"), M.mv("d7d5"), O.FIDE)
    pinned = O.fast_make(O.Pos.from_fen("8/8/8/8/k3p2Q/8/3P4/3K4 w - - 0 1"), M.mv("d2d4"), O.FIDE)
    none = O.fast_make(O.Pos(), M.mv("e2e4"), O.FIDE)
    for pos, want in ((live, True), (pinned, False), (none, False)):
        assert pos.ep >= 0
        assert M.ep_usable(pos, [int(m) for m in O.fast_gen_moves(pos, O.FIDE)]) is want


def test_in_check_and_dead():
    assert M.in_check(O.Pos.from_fen("4k3/8/8/8/8/8/8/4K2r w - - 0 1"))
    assert not M.in_check(O.Pos.from_fen("4k3/8/8/8/8/8/8/4KB1r w - - 0 1"))
    assert M.in_check(O.Pos.from_fen("4k3/8/8/8/8/8/3p4/4K3 w - - 0 1"))
    assert not M.in_check(O.Pos.from_fen("4k3/8/8/8/8/8/4p3/4K3 w - - 0 1"))
    assert M.in_check(O.Pos.from_fen("4k3/8/5N2/8/8/8/8/4K3 b - - 0 1"))
    assert M.dead(O.Pos.from_fen("4k3/8/8/8/8/8/8/4KB2 w - - 0 1"))
    assert M.dead(O.Pos.from_fen("4k1b1/8/8/8/8/8/8/4K1B1 w - - 0 1")) is False  # opposite colours
    assert M.dead(O.Pos.from_fen("4kb2/8/8/8/8/8/8/4K1B1 w - - 0 1"))  # f8 and g1: same colour
    assert not M.dead(O.Pos.from_fen("4k3/8/8/8/8/8/8/3NKN2 w - - 0 1"))
    assert not M.dead(O.Pos.from_fen("4k3/8/8/8/8/8/4P3/4K3 w - - 0 1"))
