"""CPU tests of tests/symmetry.py and of the references under it.

The GPU tests of tests/test_gpu_symmetry.py call a kernel on T(x) and expect
the existing reference's answer for x, mapped through T.  That is a test of the
kernel only if the references themselves are invariant under T: this file
checks that they are -- the fastcpu engine, the literal restatement (refcpu)
and the Python models -- and that the maps are what they say (involutions, M
and F commuting, both position forms agreeing).  No GPU."""
import json
import os

import numpy as np
import pytest

import fide_positions as FP
import oracle_lib as O
import san_model as S
import san_resolve_model as SR
import starts_batches as SB
import symmetry as Y
from symmetry import F, M, R

OG = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_golden.json")))
SUITE = [O.Pos.from_fen(e["fen"]) for e in OG["perft_fide"].values()]


def same(p, q):
    return (p.cells == q.cells).all() and (p.stm, p.castle, p.ep) == (q.stm, q.castle, q.ep)


def seeded_positions(n, seed, rules):
    """tests/test_gpu_fide.py::_fide_positions' recipe: seeded games cut at a random ply."""
    mv = O.fast_gen_games(seed, 0, n, 120, noise_per_256=0, rules=rules)
    rng = np.random.default_rng(seed)
    out = []
    for g in range(n):
        p = O.Pos()
        for ply in range(int(rng.integers(0, 120))):
            m = int(mv[ply, g])
            if m == O.SENTINEL:
                break
            if O.fast_validate(p, m, rules) == O.OK:
                p = O.fast_make(p, m, rules)
        out.append(p)
    return out


def junk_boards(n, seed):
    """Random boards of 24 pieces, kind 6 (OTHER) among them."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        cells = np.full(64, -1, np.int8)
        sq = rng.choice(64, 24, replace=False)
        cells[sq] = rng.integers(0, 2, 24) * 8 + rng.integers(0, 7, 24)
        out.append(cells)
    return out


# ------------------------------------------------------------------ the maps
def test_maps_are_involutions():
    every = np.arange(1 << 16, dtype=np.uint16)
    tok = Y.columns().tokens
    for T in Y.ALL:
        assert [T.sq(T.sq(s)) for s in range(64)] == list(range(64))
        assert (T.moves(T.moves(every)) == every).all()
        assert (T.tokens(T.tokens(tok)) == tok).all()
        for p in FP.position_set()[:100] + tuple(SUITE):
            p = p if T is F else Y.without_rights(p)
            assert same(T.pos(T.pos(p)), p)
        assert [T.result(T.result(c)) for c in range(7)] == list(range(7))
    assert [F.result(c) for c in range(7)] == [0, 2, 1, 3, 4, 5, 6] == [R.result(c) for c in range(7)]
    assert [M.result(c) for c in range(7)] == list(range(7))


def test_m_and_f_commute_to_r():
    every = np.arange(1 << 16, dtype=np.uint16)
    tok = Y.columns().tokens
    assert (M.moves(F.moves(every)) == R.moves(every)).all() and (F.moves(M.moves(every)) == R.moves(every)).all()
    assert (M.tokens(F.tokens(tok)) == R.tokens(tok)).all() and (F.tokens(M.tokens(tok)) == R.tokens(tok)).all()
    for p in FP.position_set()[:100] + tuple(SUITE):
        p = Y.without_rights(p)
        assert same(M.pos(F.pos(p)), R.pos(p)) and same(F.pos(M.pos(p)), R.pos(p))


def test_moves_is_a_bijection_on_the_plain_words():
    for T in Y.ALL:
        idx = T.words4096()
        assert sorted(idx.tolist()) == list(range(4096))
        for code in range(1, 8):  # the promotion bits are kept, codes 5-7 included
            w = np.arange(4096, dtype=np.uint16) | np.uint16(code << 12)
            assert (T.moves(w) == (idx | (code << 12))).all()
        flagged = np.arange(0x8000, 0x10000).astype(np.uint16)
        assert (T.moves(flagged) == flagged).all()
        assert T.moves(0xFFFF) == 0xFFFF and T.moves([0xFFFF, 0x8001]) == [0xFFFF, 0x8001]
    assert F.moves(12 | (28 << 6)) == 52 | (36 << 6)   # e2e4 -> e7e5
    assert M.moves(12 | (28 << 6)) == 11 | (27 << 6)   # e2e4 -> d2d4
    assert R.moves(12 | (28 << 6)) == 51 | (35 << 6)   # e2e4 -> d7d5


def test_tokens_by_hand():
    p = SR.parse
    assert F.tokens(p("Nbd2")) == p("Nbd7") and M.tokens(p("Nbd2")) == p("Nge2") ==M.tokens([p("Nbd2")])[0]
    assert F.tokens(p("R1a3")) == p("R8a6") and M.tokens(p("R1a3")) == p("R1h3") and R.tokens(p("R1a3")) == p("R8h6")
    assert R.tokens(p("Qh1e4+")) == p("Qa8d5+") and F.tokens(p("exd8=Q#")) == p("exd1=Q#")
    assert M.tokens(p("exd8=Q#")) == p("dxe8=Q#")
    for T in Y.ALL:
        for fixed in (p("O-O"), p("O-O-O+"), Y.TOKEN_NONE, 1 << 25, p("e4") | (6 << 6), p("Nf3") | (1 << 9)):
            assert T.tokens(fixed) == fixed


def test_pos_form_and_dc_pos_form_agree():
    ps = list(FP.position_set()[:80]) + SUITE + [O.Pos(c, s) for c in junk_boards(4, 3) for s in (0, 1)]
    for T in Y.ALL:
        qs = [p if T is F else Y.without_rights(p) for p in ps]
        want = SB.pos_array([T.pos(p) for p in qs])
        got = T.pos(SB.pos_array(qs))
        assert SB.same_pos(got, want).all()
        assert SB.same_pos(np.array([T.pos(SB.dpos(qs[0]))], want.dtype), want[:1]).all()
    with_rights = O.Pos()
    for T in (M, R):
        with pytest.raises(ValueError):
            T.pos(with_rights)
        with pytest.raises(ValueError):
            T.pos(SB.dpos(with_rights))
    assert Y.without_rights(with_rights).castle == 0 and with_rights.castle == 15
    assert int(Y.without_rights(SB.dpos(with_rights))["castle"]) == 0
    assert F.pos(O.Pos(with_rights.cells, 0, 0b0110, -1)).castle == 0b1001


def test_divide_and_canonical():
    d = {"796": 5, "1": 7}
    assert F.divide(d) == {str(F.moves(796)): 5, str(F.moves(1)): 7}
    assert M.divide({796: 5}) == {M.moves(796): 5}
    legal = O.fast_gen_moves(SUITE[1], O.FIDE)
    for T in Y.ALL:
        got = T.canonical(T.moves(legal))
        assert sorted(got.tolist()) == sorted(T.moves(legal).tolist())
        key = [(m & 63, (m >> 6) & 63, m >> 12) for m in got.tolist()]
        assert key == sorted(key)


# ---------------------------------------------------------------- the oracle
def oracle_positions(rules):
    return list(FP.position_set()) + seeded_positions(60, 5, rules) + SUITE


@pytest.mark.parametrize("rules", [O.REF, O.FIDE], ids=["ref", "fide"])
def test_fastcpu_is_invariant(rules):
    """fast_perft with divide at depths 1-3 and the all-pairs verdict table."""
    idx = {T: T.words4096() for T in Y.ALL}
    for p in oracle_positions(rules):
        own = {}
        for T, x, tx in Y.images(p):
            key = x.castle
            if key not in own:
                own[key] = ([O.fast_perft(x, d, rules, threads=1) for d in (1, 2, 3)], O.fast_verdicts_all(x, rules))
            perfts, verdicts = own[key]
            for d, (tot, div, rm) in zip((1, 2, 3), perfts):
                ttot, tdiv, trm = O.fast_perft(tx, d, rules, threads=1)
                assert ttot == tot, (T, d)
                assert dict(zip(trm.tolist(), tdiv.tolist())) == T.divide(dict(zip(rm.tolist(), div.tolist()))), (T, d)
            assert (O.fast_verdicts_all(tx, rules)[idx[T]] == verdicts).all(), T


def test_promotion_verdicts_are_invariant():
    """fide_positions.verdict_table, every promotion code, on the positions of the set that can promote."""
    n = 0
    for p in FP.position_set():
        if not any(int(m) >> 12 for m in O.fast_gen_moves(p, O.FIDE)):
            continue
        n += 1
        for T, x, tx in Y.images(p):
            want = FP.verdict_table(x, O.fast_gen_moves(x, O.FIDE))
            got = FP.verdict_table(tx, O.fast_gen_moves(tx, O.FIDE))
            assert (got[:, T.words4096()] == want).all(), T
            assert (want[1:] == O.OK).any()
    assert n >= 20


def test_refcpu_is_invariant():
    for cells in junk_boards(20, 5):
        assert (cells & 7 == 6).any()
        for stm in (0, 1):
            p = O.Pos(cells, stm, 0, -1)
            want = O.ref_verdicts_all(p.cells, p.stm)
            for T in Y.ALL:
                q = T.pos(p)
                assert (O.ref_verdicts_all(q.cells, q.stm)[T.words4096()] == want).all(), T


def test_published_position_4_mirrored():
    """The colour flip of position 4 is the published "Position 4 mirrored": the same counts."""
    e = OG["perft_fide"]["pos4"]
    q = F.pos(O.Pos.from_fen(e["fen"]))
    assert same(q, O.Pos.from_fen("r2q1rk1/pP1p2pp/Q4n2/bbp1p3/Np6/1B3NBn/pPPP1PPP/R3K2R b KQ - 0 1"))
    assert [O.fast_perft(q, d, O.FIDE)[0] for d in (1, 2, 3, 4, 5)] == [e["perft"][str(d)] for d in (1, 2, 3, 4, 5)]
    assert [e["perft"][str(d)] for d in (1, 2, 3, 4)] == [6, 264, 9467, 422333]


# ---------------------------------------------------------------- the models
def test_the_batch_has_its_shape():
    """What tests/test_gpu_symmetry.py relies on the batch to hold, among the unmapped columns."""
    s = Y.batch_shape()
    assert s["results"] == set(range(7))
    assert s["castles"] == {(0, "k"), (0, "q"), (1, "k"), (1, "q")}
    assert s["ep"] >= 1 and s["promos"] == {1, 2, 3, 4}
    assert {S.FILE, S.RANK, S.FILE | S.RANK} <= s["san"]
    assert {SR.NOMATCH, SR.AMBIGUOUS} <= s["words"]
    c = Y.columns()
    assert c.n == 5 * len(Y.games()) and c.moves.shape == (Y.N_PLIES, c.n)
    assert int(c.resolve_counts[1]) >= 50000  # most tokens still resolve: the junk is sparse


def test_models_are_invariant_on_the_batch():
    """san_model.annotate (outcome_model.adjudicate's dict and the SAN bytes, ply by
    ply) and san_resolve_model.walk on every mapped column against the mapped
    answers for the unmapped one."""
    c = Y.columns()
    for g in range(c.n):
        T, b = c.T[g], c.base[g]
        if T is Y.I:
            continue
        r = S.annotate(c.moves[:, g], c.starts[g], int(c.clocks[g]))
        assert r["result"] == c.result[g], (g, T)
        for k in ("end_ply", "repeats", "halfmove", "accept", "validated", "accepted", "san"):
            assert r[k] == b.game[k], (g, T, k)
        assert same(r["pos"], T.pos(b.game["pos"])), (g, T)
        words, first_bad, counts = SR.walk(c.tokens[:, g], c.starts[g])
        assert words == c.words[:, g].tolist(), (g, T)
        assert first_bad == b.first_bad and counts == b.counts, (g, T)


def test_stats_below_is_invariant():
    ps = FP.position_set()
    for p in ps[::len(ps) // 40][:40]:
        for T, x, tx in Y.images(p):
            for d in (1, 2):
                tot, rows = FP.stats_below(x, d)
                ttot, trows = FP.stats_below(tx, d)
                assert ttot == tot and trows == T.divide(rows), (T, d)
