"""CPU tests of tests/fide_positions.py: the constructed FIDE positions are
consistent, they hold the classes of position the playout sets lack (quotas on
the oracle and the models alone, no kernel involved), the third move generator
agrees with the oracle on every one of them, and the perft-statistics model
reproduces the golden tables.  tests/test_gpu_fide_constructed.py runs every
FIDE entry point over the same set."""
import collections
import functools
import json
import os

import numpy as np

import fide_positions as F
import oracle_lib as O
import san_model as S

FX = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "perft_stats.json")))

# class -> (quota, counted for constructed(640, SEED = 2025)); a quota is about
# a third of the count and never below what the set was built to hold
QUOTA = {
    "ep_legal": (48, 145),           # a legal en-passant capture exists
    "ep_two": (19, 59),              # two pawns may capture en passant
    "ep_illegal": (46, 140),         # a capturer stands there but may not (pin, exposed king, unanswered check)
    "ep_in_check": (11, 34),         # en-passant capture legal while in check
    "double_check": (20, 60),
    "single_check": (80, 242),
    "pins2": (28, 85),               # two or more pinned pieces
    "pins1": (74, 223),              # exactly one
    "castle_legal": (34, 104),
    "castle_denied": (62, 186),      # right held, king and rook at home, move denied
    "stale_right": (11, 33),         # right held whose king or rook is not at home
    "promotion": (18, 54),
    "promotion_capture": (11, 35),
    "no_moves": (6, 20),
}
TWIN_QUOTA = (34, 103)               # legal N/B/R/Q moves with a twin that reaches the square but not legally
# stats_row over every (position, legal move) of the constructed positions
STATS_QUOTA = {F.PS_DISCOVERED: (41, 123), F.PS_DOUBLE: (5, 9), F.PS_CHECKMATES: (25, 75), F.PS_STALEMATES: (7, 23),
               F.PS_EP: (68, 204), F.PS_CASTLES: (44, 133), F.PS_PROMOTIONS: (109, 328)}


@functools.lru_cache(maxsize=None)
def oracle_lists():
    return [O.fast_gen_moves(p, O.FIDE) for p in F.position_set()]


@functools.lru_cache(maxsize=None)
def all_rows():
    """(position index, move, stats_row) of every legal move of the set."""
    out = []
    for i, (p, legal) in enumerate(zip(F.position_set(), oracle_lists())):
        out += [(i, int(m), r) for m, r in zip(legal, F.stats_rows(p, legal))]
    return out


def test_constructed_positions_are_consistent():
    ps = F.position_set()[:F.N_CONSTRUCTED]
    assert len(ps) == 640
    assert all(F.consistent(p) for p in ps)
    assert all(F.consistent(p) for p in F.hand_positions())
    assert max(len(m) for m in oracle_lists()) < 256
    stm = collections.Counter(p.stm for p in ps)
    assert stm[0] >= 200 and stm[1] >= 200
    # deterministic: the same seed gives the same boards, another seed others
    again = F.constructed(40, F.SEED)
    assert all((a.cells == b.cells).all() and (a.stm, a.castle, a.ep) == (b.stm, b.castle, b.ep)
               for a, b in zip(again, ps))
    other = F.constructed(40, F.SEED + 1)
    assert any((a.cells != b.cells).any() for a, b in zip(other, ps))


def test_inconsistent_positions_are_recognised():
    p = O.Pos.from_fen("4k3/8/8/8/3Pp3/8/8/4K3 b - d3 0 1")
    assert F.consistent(p)
    for fen in ("4k3/8/8/8/3Pp3/8/8/4K3 b - e3 0 1",     # no pawn in front of the ep square
                "4k3/8/8/8/3Pp3/8/3N4/4K3 b - d3 0 1",    # the pawn's origin square is occupied
                "8/8/8/8/8/8/4k3/4K3 w - - 0 1",          # adjacent kings
                "4k3/8/8/8/8/8/8/P3K3 w - - 0 1",         # a pawn on the first rank
                "4k3/8/8/8/8/8/8/4K2r b - - 0 1",         # the side not to move is in check
                "4k3/8/8/8/8/8/8/8 w - - 0 1"):           # no white king
        assert not F.consistent(O.Pos.from_fen(fen)), fen


def test_coverage_quotas():
    ps = F.position_set()[:F.N_CONSTRUCTED]
    cnt = collections.Counter()
    twins = 0
    for p, legal in zip(ps, oracle_lists()):
        for k, v in F.features(p, legal).items():
            cnt[k] += bool(v)
        twins += F.twin_illegal(p, legal)
    print({k: cnt[k] for k in QUOTA}, "twin_illegal", twins)
    for k, (quota, counted) in QUOTA.items():
        assert cnt[k] == counted, (k, cnt[k], counted)  # the figures written above are the measured ones
        assert counted >= quota, k
    assert twins == TWIN_QUOTA[1] >= TWIN_QUOTA[0]
    floor = {"ep_legal": 40, "ep_two": 15, "ep_illegal": 20, "ep_in_check": 8, "double_check": 10, "pins2": 8,
             "pins1": 40, "castle_legal": 30, "castle_denied": 30, "stale_right": 10, "promotion": 15,
             "promotion_capture": 4, "no_moves": 3}
    assert all(QUOTA[k][0] >= v for k, v in floor.items()) and TWIN_QUOTA[0] >= 8


def test_move_class_quotas():
    n = F.N_CONSTRUCTED
    tot = np.zeros(F.PS_COUNT, np.int64)
    for i, _, r in all_rows():
        if i < n:
            tot += r
    print(tot.tolist())
    for k, (quota, counted) in STATS_QUOTA.items():
        assert int(tot[k]) == counted, (k, int(tot[k]), counted)
        assert counted >= quota >= 5, k
    # over the whole set (the hand-made positions supply what the generator may not)
    rows = [r for _, _, r in all_rows()]
    assert sum(r[F.PS_EP] and r[F.PS_DISCOVERED] for r in rows) >= 1
    assert sum(r[F.PS_CASTLES] and r[F.PS_CHECKS] for r in rows) >= 1
    assert sum(r[F.PS_PROMOTIONS] and r[F.PS_CHECKS] for r in rows) >= 1
    assert not any(r[F.PS_KING_CAPTURES] for r in rows)


def test_hand_made_positions():
    for (fen, count, why), p in zip(F.HAND, F.hand_positions()):
        assert len(O.fast_gen_moves(p, O.FIDE)) == len(F.py_legal_moves(p)) == count, fen
    # the en-passant discovery, the checking castle and the checking promotion, each by name
    by_fen = {fen: p for (fen, _, _), p in zip(F.HAND, F.hand_positions())}
    r = F.stats_row(by_fen["8/8/8/R2pP2k/8/8/8/4K3 w - d6 0 1"], S.M.mv("e5d6"))
    assert r[F.PS_EP] and r[F.PS_CAPTURES] and r[F.PS_CHECKS] and r[F.PS_DISCOVERED] and not r[F.PS_DOUBLE]
    r = F.stats_row(by_fen["5k2/8/8/8/8/8/8/4K2R w K - 0 1"], S.M.mv("e1g1"))
    assert r[F.PS_CASTLES] and r[F.PS_CHECKS] and not r[F.PS_DISCOVERED]
    r = F.stats_row(by_fen["4k3/P7/8/8/8/8/8/4K3 w - - 0 1"], S.M.mv("a7a8q"))
    assert r[F.PS_PROMOTIONS] and r[F.PS_CHECKS] and not r[F.PS_DISCOVERED]
    r = F.stats_row(by_fen["4k3/8/4N3/8/8/8/8/4RK2 w - - 0 1"], S.M.mv("e6c7"))
    assert r[F.PS_CHECKS] and r[F.PS_DOUBLE] and not r[F.PS_DISCOVERED]
    # en passant: excluded where it exposes the king, an evasion where the pushed pawn checks
    assert S.M.mv("e4d3") not in F.py_legal_moves(by_fen["8/8/8/8/k2Pp2Q/8/8/3K4 b - d3 0 1"])
    p = by_fen["8/8/8/2k5/3Pp3/8/8/4K3 b - d3 0 1"]
    assert F.in_check(p) and S.M.mv("e4d3") in F.py_legal_moves(p)
    assert F.features(p, F.py_legal_moves(p))["ep_in_check"]


def test_three_queens_need_file_and_rank():
    p = O.Pos.from_fen("8/k7/8/8/7Q/8/8/K3Q2Q w - - 0 1")
    legal = [int(m) for m in O.fast_gen_moves(p, O.FIDE)]
    want = {"h1e4": S.FILE | S.RANK, "h4e4": S.RANK, "e1e4": S.FILE}
    for text, flags in want.items():
        m = S.M.mv(text)
        child = O.fast_make(p, m, O.FIDE)
        byte = S.san_byte(p, legal, m, child, [int(x) for x in O.fast_gen_moves(child, O.FIDE)])
        assert byte & (S.FILE | S.RANK) == flags and byte & 7 == F.Q, text
    assert S.san_text(S.M.mv("h1e4"), F.Q | S.FILE | S.RANK) == "Qh1e4"


def test_py_legal_moves_equals_the_oracle():
    for i, (p, legal) in enumerate(zip(F.position_set(), oracle_lists())):
        assert F.py_legal_moves(p) == [int(m) for m in legal], i
    # ... and on the suite positions, the start position among them
    for e in FX["fide_suite"].values():
        p = O.Pos.from_fen(e["fen"])
        assert F.py_legal_moves(p) == [int(m) for m in O.fast_gen_moves(p, O.FIDE)], e["fen"]


def test_py_make_equals_the_oracle():
    n = 0
    for p, legal in zip(F.position_set(), oracle_lists()):
        for m in legal[:6]:
            a, b = F.py_make(p, int(m)), O.fast_make(p, int(m), O.FIDE)
            assert (a.cells == b.cells).all() and (a.stm, a.castle, a.ep) == (b.stm, b.castle, b.ep)
            n += 1
    assert n > 3000


def test_in_check_equals_the_outcome_model():
    for p in F.position_set():
        assert F.in_check(p) == S.M.in_check(p)


def _by_move(moves, rows):
    return {int(m): [int(v) for v in r] for m, r in zip(moves, rows)}


def test_stats_row_reproduces_the_golden_depth1():
    entries = list(FX["fide_small"]) + list(FX["fide_suite"].values())
    assert len(entries) == 13
    for e in entries:
        totals, rows = F.stats_below(O.Pos.from_fen(e["fen"]), 1)
        g = e["depths"]["1"]
        assert totals == g["totals"], e["fen"]
        if "rows" in g:
            assert rows == _by_move(g["moves"], g["rows"]), e["fen"]
    assert all("rows" in e["depths"]["1"] for e in FX["fide_small"])


def test_stats_row_reproduces_the_golden_depth2():
    for e in FX["fide_small"]:
        totals, rows = F.stats_below(O.Pos.from_fen(e["fen"]), 2)
        g = e["depths"]["2"]
        assert totals == g["totals"], e["fen"]
        assert rows == _by_move(g["moves"], g["rows"]), e["fen"]
    # two suite positions as well: castles, promotions and en passant at the second ply
    for name in ("kiwipete", "pos4", "pos3"):
        e = FX["fide_suite"][name]
        assert F.stats_below(O.Pos.from_fen(e["fen"]), 2)[0] == e["depths"]["2"]["totals"], name
