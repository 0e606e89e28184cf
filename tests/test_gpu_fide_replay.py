"""GPU tests of the plain FIDE replay and the FIDE game generator
(k_replay_fide and k_gen_games_fide: dc_replay / dc_replay_device /
dc_gen_games / dc_gen_games_device / dc_multi_replay with DC_RULES_FIDE) at
their edges.  Every comparison is exact; the expected values are the fastcpu
oracle's or the hand-written accept strings of tests/fide_scripts.py.  The
moves that are replayed come from the oracle or are built on the host
(tests/fide_replay_batches.py), never from the kernel under test;
tests/test_fide_replay_model.py asserts what those inputs hold.

The digest leaves castling rights and the en-passant square out, so a wrong
right or a stale square shows only in a later accept bit: that is what the
scripted games are for.  The FIDE rule code takes wave-wide shortcuts, and in
a replay every lane holds another game at another stage: the same games are
therefore also replayed in another order and alone."""
import numpy as np
import pytest

import dchess
import dchess.dist as D
import fide_replay_batches as B
import fide_scripts as S
import oracle_lib as O
from test_gpu_legal_moves import dpos

pytestmark = pytest.mark.gpu

FIDE = dchess.RULES_FIDE
NONE = dchess.MOVE_NONE
GROUPS = S.groups()


def stats_list(st):
    return [st[k] for k in D.STAT_KEYS]


def bits(bitmap, n_games):
    """(accept bits [n_plies, n_games], the bits of the last word at or past n_games)."""
    b = np.unpackbits(np.ascontiguousarray(bitmap).view(np.uint8).reshape(bitmap.shape[0], -1), axis=1,
                      bitorder="little")
    return b[:, :n_games], b[:, n_games:]


def same_as_oracle(got, want, n_games):
    (bm, dg, st), (fbm, fdg, fst) = got, want
    assert bm.shape == fbm.shape and (bm == fbm).all()
    assert (dg == fdg).all()
    assert stats_list(st) == [int(x) for x in fst]
    assert not bits(bm, n_games)[1].any()


def replay_ok(engine, mv, start=None):
    """One FIDE replay checked against the oracle's from the same start."""
    got = engine.replay(mv, rules=FIDE, start=None if start is None else dpos(start))
    same_as_oracle(got, O.fast_replay(mv, O.FIDE, start=start), mv.shape[1])
    return got


# ---------------------------------------------------------------- scripted games
@pytest.mark.parametrize("k", range(len(GROUPS)), ids=[g[0].name for _, g in GROUPS])
def test_scripted_games(engine, k):
    """The scripts of one start in one call (1 to 8 games): accept columns equal
    the hand-written strings, the counters their sums, the digests the oracle's
    final boards'."""
    fen, scripts = GROUPS[k]
    start = O.Pos() if fen is None else O.Pos.from_fen(fen)
    mv = S.matrix(scripts)
    bm, dg, st = engine.replay(mv, rules=FIDE, start=None if fen is None else dpos(start))
    got = [S.column_bits(bm, mv, g, len(s.bits)) for g, s in enumerate(scripts)]
    assert got == [s.bits for s in scripts], [s.name for s, g in zip(scripts, got) if s.bits != g]
    assert not bits(bm, len(scripts))[0][mv == NONE].any() and not bits(bm, len(scripts))[1].any()
    ones = sum(s.bits.count("1") for s in scripts)
    zeros = sum(s.bits.count("0") for s in scripts)
    assert (st["validated"], st["accepted"], st["rejected"]) == (ones + zeros, ones, zeros)
    for g, s in enumerate(scripts):
        p = start.copy()
        for m in S.words(s):
            if m != NONE and O.fast_validate(p, m, O.FIDE) == O.OK:
                p = O.fast_make(p, m, O.FIDE)
        assert int(dg[g]) == O.digest(p.cells, p.stm), s.name
    assert st["digest_sum"] == int(dg.sum(dtype=np.uint64)) and st["digest_xor"] == int(np.bitwise_xor.reduce(dg))


# ------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("n_games,n_plies,noise", B.RAGGED)
def test_replay_ragged_vs_fastcpu(engine, n_games, n_plies, noise):
    """One game, 63/64/65, the 256-thread block edge, a partly filled last word."""
    replay_ok(engine, B.ragged(n_games, n_plies, noise))


def test_replay_full_16_bit_words(engine):
    """Random 16-bit words, promotion codes added, removed and set to 5..7,
    flagged legal moves and DC_MOVE_NONE in mid-game."""
    mv, _ = B.junk_batch()
    bm, dg, st = replay_ok(engine, mv)
    assert st["validated"] == int((mv != NONE).sum())
    assert not bits(bm, mv.shape[1])[0][(mv & 0x8000) != 0].any()  # flagged or none: never accepted


def test_replay_from_custom_starts(engine):
    """start != NULL: Black to move, en-passant squares, each single castling
    right, the suite FENs; the moves that need the start's castle and ep fields
    are first plies of every batch."""
    starts = B.custom_starts()
    assert len(starts) >= B.N_FROM_SET + 6
    for i, (label, start) in enumerate(starts):
        mv = B.games_from(i)
        got = engine.replay(mv, rules=FIDE, start=dpos(start))
        want = O.fast_replay(mv, O.FIDE, start=start)
        bad = np.flatnonzero((bits(got[0], 64)[0] != bits(want[0], 64)[0]).any(axis=0))
        assert not len(bad), (label, bad[:4].tolist())
        same_as_oracle(got, want, 64)


def test_replay_edge_calls(engine):
    black = O.Pos.from_fen(S.BISHOP)
    # no plies: the digests are the start's, nothing is counted
    for start in (None, black):
        p = start or O.Pos()
        bm, dg, st = engine.replay(np.zeros((0, 70), np.uint16), rules=FIDE, start=None if start is None else dpos(p))
        d = O.digest(p.cells, p.stm)
        assert bm.shape == (0, 2) and (dg == d).all()
        assert (st["validated"], st["accepted"], st["rejected"]) == (0, 0, 0)
        assert st["digest_sum"] == (70 * d) % 2**64 and st["digest_xor"] == 0
        # only DC_MOVE_NONE: the same, with an all-zero bitmap
        bm, dg, st2 = engine.replay(np.full((5, 70), NONE, np.uint16), rules=FIDE,
                                    start=None if start is None else dpos(p))
        assert bm.shape == (5, 2) and not bm.any() and (dg == d).all() and st2 == st
    # the outputs are optional and the counters do not depend on them
    mv, _ = B.junk_batch()
    bm, dg, st = engine.replay(mv, rules=FIDE)
    for want_bitmap, want_digests in ((False, True), (True, False), (False, False)):
        bm2, dg2, st2 = engine.replay(mv, rules=FIDE, want_bitmap=want_bitmap, want_digests=want_digests)
        assert st2 == st
        assert (bm2 is None) == (not want_bitmap) and (dg2 is None) == (not want_digests)
        assert bm2 is None or (bm2 == bm).all()
        assert dg2 is None or (dg2 == dg).all()
    bad = dpos(black)
    bad["stm"] = 2
    with pytest.raises(dchess.DChessError) as e:
        engine.replay(mv, rules=FIDE, start=bad)
    assert e.value.status == dchess.EINVAL


def test_replay_device_form(engine):
    """dc_replay_device gives what dc_replay gives, for 257 games."""
    mv = B.games(*B.GEN_TABLE[1])
    n_plies, n_games = mv.shape
    assert n_games == 257
    words = (n_games + 63) // 64
    bm, dg, st = replay_ok(engine, mv)
    d_moves, d_bm, d_dg = engine.alloc(mv.nbytes), engine.alloc(words * n_plies * 8), engine.alloc(n_games * 8)
    try:
        d_moves.upload(mv)
        dst = engine.replay_device(d_moves, n_games, n_plies, d_bm, d_dg, rules=FIDE)
        assert dst == st
        assert (d_bm.download(np.uint64, words * n_plies).reshape(n_plies, words) == bm).all()
        assert (d_dg.download(np.uint64, n_games) == dg).all()
        assert engine.replay_device(d_moves, n_games, n_plies, None, None, rules=FIDE) == st
    finally:
        for b in (d_moves, d_bm, d_dg):
            b.free()


# ------------------------------------------------------- neighbour independence
def test_replay_does_not_depend_on_the_neighbours(engine):
    mv = B.games(*B.BIG)
    n_plies, n_games = mv.shape
    fbm, fdg, fst = O.fast_replay(mv, O.FIDE)
    want = bits(fbm, n_games)[0]
    perm = np.random.default_rng(17).permutation(n_games)
    bm, dg, st = engine.replay(np.ascontiguousarray(mv[:, perm]), rules=FIDE)
    assert (bits(bm, n_games)[0] == want[:, perm]).all()
    assert (dg == fdg[perm]).all()
    assert stats_list(st) == [int(x) for x in fst]


def test_replay_of_a_game_alone(engine):
    """Sixteen columns of the 512 x 400 batch, n_games = 1 each: games that end
    early, castle, promote and capture en passant."""
    mv = B.games(*B.BIG)
    fbm, fdg, _ = O.fast_replay(mv, O.FIDE)
    want = bits(fbm, mv.shape[1])[0]
    walk = B.big_walk()
    for g in B.lone_columns():
        bm, dg, st = engine.replay(np.ascontiguousarray(mv[:, g:g + 1]), rules=FIDE)
        assert bm.shape == (mv.shape[0], 1) and (bm[:, 0] == want[:, g]).all(), g
        assert int(dg[0]) == int(fdg[g]), g
        end = int(walk["end"][g])
        assert stats_list(st) == [end, end, 0, int(fdg[g]), int(fdg[g])], g


def test_replay_equals_apply_batch_ply_by_ply(engine):
    mv = B.games(*B.APPLIED)
    n_plies, n_games = mv.shape
    bm, dg, st = replay_ok(engine, mv)
    pos = np.array([dchess.startpos()] * n_games, dchess.POS_DTYPE)
    ok = np.zeros((n_plies, n_games), np.uint8)
    for ply in range(n_plies):
        pos, ver, _ = engine.apply_batch(pos, mv[ply], rules=FIDE)
        ok[ply] = ver == dchess.V_OK
    assert (ok == bits(bm, n_games)[0]).all()
    for g in range(n_games):
        cells, stm = dchess.pos_to_cells(pos[g])
        assert O.digest(cells, stm) == int(dg[g]), g
    assert st["accepted"] == int(ok.sum())


# ------------------------------------------------------------------------ shards
def test_replay_shards_fold_and_scatter(engine):
    """The replay shard contract under FIDE: three dc_replay_shard_range ranges
    replayed alone fold to the whole batch's counters; their bitmaps, placed by
    word column and through dc_replay_scatter_shards, are the whole bitmap."""
    mv = B.games(*B.SHARDED)
    n_plies, n_games = mv.shape
    assert n_games == 1000
    bm, dg, st = replay_ok(engine, mv)
    words = (n_games + 63) // 64
    per = (words + 2) // 3
    placed = np.zeros((n_plies, words), np.uint64)
    gathered = np.zeros((3, n_plies, per), np.uint64)
    recs, covered = [], 0
    for s in range(3):
        first, cnt = dchess.replay_shard_range(n_games, s, 3)
        assert first == covered and first % 64 == 0 and cnt > 0
        covered += cnt
        w = (cnt + 63) // 64
        sbm, sdg, sst = engine.replay(np.ascontiguousarray(mv[:, first:first + cnt]), rules=FIDE)
        assert (sdg == dg[first:first + cnt]).all()
        placed[:, first // 64:first // 64 + w] = sbm
        gathered[s, :, :w] = sbm
        recs.append(stats_list(sst))
    assert covered == n_games
    assert D.fold_stats(recs) == st
    assert (placed == bm).all()
    out = np.zeros((n_plies, words), np.uint64)
    assert dchess.lib().dc_replay_scatter_shards(n_games, 3, n_plies, gathered.ctypes.data, out.ctypes.data) == 0
    assert (out == bm).all()


def test_multi_replay_fide_single_device():
    """dc_multi_replay under FIDE over one device vs fastcpu, ragged size."""
    seed, n, plies = 0xF1DE, 10_003, 60
    bm, st = dchess.multi_replay([0], seed, n, plies, 32, rules=FIDE)
    fbm, _, fst = O.fast_replay(B.games(seed, 0, n, plies, 32), O.FIDE)
    assert (bm == fbm).all()
    assert stats_list(st) == [int(x) for x in fst]
    assert int(fst[2]) > 0 and not bits(bm, n)[1].any()


# --------------------------------------------------------------------- generator
@pytest.mark.parametrize("seed,first_game,n_games,n_plies,noise", B.GEN_TABLE)
def test_gen_games_equals_fastcpu(engine, seed, first_game, n_games, n_plies, noise):
    mv = engine.gen_games(seed, first_game, n_games, n_plies, noise, rules=FIDE)
    want = B.games(seed, first_game, n_games, n_plies, noise)
    bad = np.flatnonzero((mv != want).any(axis=0))
    assert not len(bad), bad[:8].tolist()


def test_gen_games_arguments(engine):
    with pytest.raises(dchess.DChessError) as e:
        engine.gen_games(1, 0, 4, 4, 257, rules=FIDE)
    assert e.value.status == dchess.EINVAL
    assert engine.gen_games(1, 0, 0, 8, 0, rules=FIDE).shape == (8, 0)
    assert engine.gen_games(1, 0, 8, 0, 0, rules=FIDE).shape == (0, 8)
    # no games or no plies: success, and not a word written
    buf = engine.alloc(64 * 2)
    try:
        buf.upload(np.full(64, 0xABCD, np.uint16))
        engine.gen_games_device(buf, 1, 0, 0, 8, 0, rules=FIDE)
        engine.gen_games_device(buf, 1, 0, 8, 0, 0, rules=FIDE)
        assert (buf.download(np.uint16, 64) == 0xABCD).all()
        with pytest.raises(dchess.DChessError) as e:
            engine.gen_games_device(buf, 1, 0, 8, 8, 300, rules=FIDE)
        assert e.value.status == dchess.EINVAL
        assert (buf.download(np.uint16, 64) == 0xABCD).all()
    finally:
        buf.free()


def test_gen_games_sentinel_tails(engine):
    """After mate or stalemate the rest of a game is DC_MOVE_NONE, from the ply the oracle's game ends at."""
    seed, first, n_games, n_plies, noise = B.BIG
    mv = engine.gen_games(seed, first, n_games, n_plies, noise, rules=FIDE)
    none = mv == NONE
    assert (none[:-1] <= none[1:]).all()  # once DC_MOVE_NONE, only that
    end = np.where(none.any(axis=0), none.argmax(axis=0), n_plies)
    assert (end == B.big_walk()["end"]).all()
    assert int((end < n_plies).sum()) == 110 and int(end.min()) == 38
    # with noise words: an ended game draws no more of them
    seed, first, n_games, n_plies, noise = B.GEN_TABLE[1]
    none = engine.gen_games(seed, first, n_games, n_plies, noise, rules=FIDE) == NONE
    want = B.games(*B.GEN_TABLE[1]) == NONE
    assert (none[:-1] <= none[1:]).all() and (none.argmax(axis=0) == want.argmax(axis=0)).all()
    assert (none[-1] == want[-1]).all() and int(none[-1].sum()) == 52


def test_gen_games_first_game_composes(engine):
    """Games [a, a + n) generated alone are columns [a, a + n) of [0, N)."""
    seed, _, n_total, n_plies, noise = B.BIG
    whole = B.games(*B.BIG)
    ranges = [(5, 60), (63, 2), (100, 257), (255, 257), (511, 1)]
    ranges += [dchess.replay_shard_range(n_total, s, 3) for s in range(3)]
    assert sum(c for _, c in ranges[-3:]) == n_total
    for a, n in ranges:
        part = engine.gen_games(seed, a, n, n_plies, noise, rules=FIDE)
        assert (part == whole[:, a:a + n]).all(), (a, n)
    seed, _, n_total, n_plies, noise = B.GEN_TABLE[1]  # with noise words
    part = engine.gen_games(seed, 130, n_total - 130, n_plies, noise, rules=FIDE)
    assert (part == B.games(*B.GEN_TABLE[1])[:, 130:]).all()


def test_gen_games_device_form(engine):
    seed, first, n_games, n_plies, noise = B.MID
    d_out = engine.alloc(n_games * n_plies * 2)
    try:
        engine.gen_games_device(d_out, seed, first, n_games, n_plies, noise, rules=FIDE)
        dev = d_out.download(np.uint16, n_games * n_plies).reshape(n_plies, n_games)
    finally:
        d_out.free()
    assert (dev == engine.gen_games(seed, first, n_games, n_plies, noise, rules=FIDE)).all()
    assert (dev == B.games(*B.MID)).all()


@pytest.mark.parametrize("batch", [B.MID, B.BIG], ids=["128x300", "512x400"])
def test_generated_moves_are_all_accepted(engine, batch):
    """Every word the generator emits at noise 0 is a legal move of its game."""
    seed, first, n_games, n_plies, noise = batch
    assert noise == 0
    mv = engine.gen_games(seed, first, n_games, n_plies, noise, rules=FIDE)
    _, _, st = engine.replay(mv, rules=FIDE)
    assert st["accepted"] == st["validated"] == int((mv != NONE).sum()) and st["rejected"] == 0
