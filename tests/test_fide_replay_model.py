"""CPU tests of the inputs of tests/test_gpu_fide_replay.py: the hand-written
accept strings of tests/fide_scripts.py agree with the fastcpu oracle, move by
move and through its replay from a given start, and the seeded batches of
tests/fide_replay_batches.py hold what the GPU tests rely on -- ended games,
both castles, en passant, every promotion code, junk that leaves the games
moving, custom starts of every kind.  No kernel is involved."""
import numpy as np
import pytest

import fide_positions as F
import fide_replay_batches as B
import fide_scripts as S
import oracle_lib as O

# king-side castles, queen-side castles and en-passant captures of the two noise-0 batches, as counted
BIG_CASTLES_EP = (28, 10, 9)
MID_CASTLES_EP = (8, 4, 4)


def start_of(fen):
    return O.Pos() if fen is None else O.Pos.from_fen(fen)


def test_move_text():
    assert S.word("e2e4") == 12 | (28 << 6)
    assert S.word("a7a8=3") == 48 | (56 << 6) | (3 << 12)
    assert S.word("e7e5!") == 0x8000 | 52 | (36 << 6)
    assert S.word("--") == S.NONE == O.SENTINEL
    assert len({s.name for s in S.ALL}) == len(S.ALL) == 8 + 12 + 8 + 24
    for s in S.ALL:
        assert len(S.words(s)) == len(s.bits) and set(s.bits) <= set("01."), s.name
        assert [w == S.NONE for w in S.words(s)] == [b == "." for b in s.bits], s.name
    # one call per start: groups of 1 to 8 games
    sizes = [len(g) for _, g in S.groups()]
    assert min(sizes) == 1 and max(sizes) == 8 and sum(sizes) == len(S.ALL)


@pytest.mark.parametrize("script", S.ALL, ids=[s.name for s in S.ALL])
def test_script_move_by_move(script):
    """fast_validate / fast_make give the hand-written string, its count and the final rights and ep square."""
    p = start_of(script.fen)
    got, n = "", 0
    for m in S.words(script):
        if m == S.NONE:
            got += "."
            continue
        n += 1
        ok = O.fast_validate(p, m, O.FIDE) == O.OK
        got += "1" if ok else "0"
        if ok:
            p = O.fast_make(p, m, O.FIDE)
    assert got == script.bits
    assert n == S.validated(script)
    assert (p.castle, p.ep) == (script.castle, script.ep)


def test_scripts_through_replay_from():
    """or_fast_replay_from over each start's matrix: accept columns, counters and digests."""
    for fen, scripts in S.groups():
        start = start_of(fen)
        mv = S.matrix(scripts)
        bm, dg, st = O.fast_replay(mv, O.FIDE, start=start)
        assert [S.column_bits(bm, mv, g, len(s.bits)) for g, s in enumerate(scripts)] == [s.bits for s in scripts], fen
        ones = sum(s.bits.count("1") for s in scripts)
        zeros = sum(s.bits.count("0") for s in scripts)
        assert [int(x) for x in st[:3]] == [ones + zeros, ones, zeros], fen
        for g, s in enumerate(scripts):
            p = start.copy()
            for m in S.words(s):
                if m != S.NONE and O.fast_validate(p, m, O.FIDE) == O.OK:
                    p = O.fast_make(p, m, O.FIDE)
            assert int(dg[g]) == O.digest(p.cells, p.stm), s.name
        if fen is None:  # the default start is the start position
            dbm, ddg, dst = O.fast_replay(mv, O.FIDE)
            assert (dbm == bm).all() and (ddg == dg).all() and (dst == st).all()


def test_castle_scripts_follow_the_rights():
    assert len(S.CASTLES) == 24 and sum(s.bits == "1" for s in S.CASTLES) == 8
    by = {s.name: s for s in S.CASTLES}
    assert by["rights_KQkq_w_e1g1"].castle == 12 and by["rights_KQkq_b_e8g8"].castle == 3
    assert by["rights_K_w_e1g1"].bits == "1" and by["rights_K_w_e1c1"].bits == "0"
    assert by["rights_k_w_e1g1"].bits == "0" and by["rights_k_w_e1g1"].castle == 4
    assert all(s.bits == "0" for s in S.CASTLES if "_-_" in s.name)


# ------------------------------------------------------------ seeded batches
def test_big_batch_holds_every_kind_of_move():
    mv = B.games(*B.BIG)
    w = B.big_walk()
    n_plies = B.BIG[3]
    ended = w["end"] < n_plies
    print(int(ended.sum()), int(w["end"].min()), w["promo"].sum(axis=0).tolist(), int(w["castle_k"].sum()),
          int(w["castle_q"].sum()), int(w["ep"].sum()))
    assert int(ended.sum()) == 110 and int(w["end"].min()) == 38
    assert w["promo"].sum(axis=0).tolist() == [0, 311, 353, 339, 318]
    assert (int(w["castle_k"].sum()), int(w["castle_q"].sum()), int(w["ep"].sum())) == BIG_CASTLES_EP
    assert min(BIG_CASTLES_EP) >= 1
    # the walk that counted them ends on the oracle's boards, and the oracle accepts every word
    bm, dg, st = O.fast_replay(mv, O.FIDE)
    assert (dg == w["digest"]).all()
    assert int(st[0]) == int(st[1]) == int(w["end"].sum()) and int(st[2]) == 0


def test_mid_batch_castles_and_captures_en_passant():
    w = B.walk(B.games(*B.MID))
    got = (int(w["castle_k"].sum()), int(w["castle_q"].sum()), int(w["ep"].sum()))
    print(got)
    assert got == MID_CASTLES_EP
    assert got[0] + got[1] == 12 and got[2] == 4 and min(got) >= 1


def test_lone_columns_cover_the_kinds():
    cols = B.lone_columns()
    w = B.big_walk()[cols]
    assert len(set(cols)) == B.N_LONE == 16
    assert (w["end"] < B.BIG[3]).sum() >= 4 and w["end"].min() == 38
    assert ((w["castle_k"] + w["castle_q"]) > 0).sum() >= 4
    assert (w["promo"].sum(axis=1) > 0).sum() >= 4 and (w["ep"] > 0).sum() >= 1


def test_ragged_batches_are_not_trivial():
    for n_games, n_plies, noise in B.RAGGED:
        mv = B.ragged(n_games, n_plies, noise)
        assert mv.shape == (n_plies, n_games)
        _, _, st = O.fast_replay(mv, O.FIDE)
        assert int(st[0]) > 0 and (noise == 255 or 2 * int(st[1]) >= int(st[0]))
        assert (int(st[2]) > 0) == (noise > 0), (n_games, noise)
    mv = B.ragged(257, 30, 255)
    _, _, st = O.fast_replay(mv, O.FIDE)
    assert 0 < int(st[1]) < int(st[2])  # nearly all noise, yet some games move


def test_noisy_batches_hold_ended_games():
    """Games that end among noise words: 52 of the generator table's 257 x 600
    batch (the earliest at ply 46), and some of the sharded and the 10,003-game
    batches; once a column holds DC_MOVE_NONE it holds only that."""
    none = B.games(*B.GEN_TABLE[1]) == S.NONE
    assert (none[:-1] <= none[1:]).all()
    assert int(none[-1].sum()) == 52 and int(np.where(none.any(axis=0), none.argmax(axis=0), 600).min()) == 46
    assert int((B.games(*B.SHARDED)[-1] == S.NONE).sum()) == 8
    assert int((B.games(0xF1DE, 0, 10_003, 60, 32)[-1] == S.NONE).sum()) == 98


def test_junk_batch_keeps_moving():
    mv, what = B.junk_batch()
    n_plies, n_games = mv.shape
    assert (n_games, n_plies) == (200, 60)
    print(dict(what))
    bm, dg, st = O.fast_replay(mv, O.FIDE)
    # the cap: at least half of all plies are still accepted
    assert int(st[1]) >= n_games * n_plies // 2
    written = sum(what[k] for k in ("random", "code_added", "code_removed", "code_5_to_7", "flagged", "none"))
    assert 0.25 * mv.size <= written <= 0.35 * mv.size
    # a quarter of the overwritten plies each: 900 expected, and 4/7 and 3/7 of 900 for the two code changes
    assert min(what["random"], what["code_added"], what["code_5_to_7"], what["flagged"], what["none"]) >= 300
    # promotions are rare in 60 plies: the ones played are counted here, the ones with the code taken away are
    # first plies of the custom starts (below) and the promote_code_0 script
    assert what["promotion_played"] >= 1
    # DC_MOVE_NONE stands in mid-game: moves follow it in its column
    after = np.flip(np.maximum.accumulate(np.flip(mv != S.NONE, axis=0), axis=0), axis=0)
    assert int(((mv == S.NONE) & after).sum()) >= 400
    assert int(((mv >= 0x8000) & (mv != S.NONE)).sum()) >= what["flagged"]
    # every overwritten word but a lucky random one is rejected, DC_MOVE_NONE is not counted
    assert int(st[0]) == int((mv != S.NONE).sum())
    assert int(st[2]) >= written - what["none"] - what["random"]


def test_custom_starts_cover_the_start_fields():
    starts = B.custom_starts()
    from_set = [(label, p) for label, p in starts if not label.startswith("suite_")]
    assert len(from_set) >= 24 and len(starts) == len(from_set) + 6
    assert sum(p.stm == 1 for _, p in from_set) >= 6 and sum(p.stm == 0 for _, p in from_set) >= 6
    assert {p.castle for _, p in from_set} >= {0, 1, 2, 4, 8}
    assert sum(p.ep >= 0 for _, p in from_set) >= 6
    played_ep = played_castle = played_promo = spoiled = 0
    for i, (label, p) in enumerate(starts):
        legal = [int(m) for m in O.fast_gen_moves(p, O.FIDE)]
        feat = F.features(p, legal)
        mv = B.games_from(i)
        assert mv.shape == (30, 64)
        first = set(int(m) for m in mv[0])
        castles = [m for m in legal if (int(p.cells[m & 63]) & 7) == F.K and abs((m & 63) - ((m >> 6) & 63)) == 2]
        caps = [m for m in legal if (int(p.cells[m & 63]) & 7) == F.P and (m >> 6) & 63 == p.ep]
        promos = [m for m in legal if m >> 12]
        # the moves that need the start's castle and ep fields are all first plies
        assert set(castles) | set(caps) <= first, label
        assert bool(castles) == feat["castle_legal"] and bool(caps) == feat["ep_legal"], label
        if label.startswith("only_right"):
            assert len(castles) == 1 and p.castle in (1, 2, 4, 8), label
        played_castle += bool(castles)
        played_ep += bool(caps)
        played_promo += any(m in first for m in promos)
        # a promotion with its code taken away, and with one that names no piece
        spoiled += any(m & 0xFFF in first for m in promos) and any((m & 0xFFF) | (6 << 12) in first for m in promos)
        bm, dg, st = O.fast_replay(mv, O.FIDE, start=p)
        if legal:
            assert int(st[1]) >= int(st[0]) // 4 and int(st[2]) > 0, label
        else:
            assert int(st[1]) == 0 and int(st[0]) > 0, label
        assert (mv == S.NONE).any() and ((mv >= 0x8000) & (mv != S.NONE)).any(), label
    print(played_ep, played_castle, played_promo, spoiled)
    assert played_ep >= 6 and played_castle >= 8 and played_promo >= 4 and spoiled >= 3
