"""GPU tests of the per-game-start calls -- dc_replay_outcome_starts,
dc_replay_san_starts, dc_san_resolve_starts and their _device forms -- against
the shared-start calls (GPU against GPU, bit for bit) and against the
oracle-backed models, one model call per game with that game's own start and
clock (tests/starts_batches.py; tests/test_starts_model.py says what the batches
hold).  Everything is integer and compared exactly."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import dchess
import fide_replay_batches as FB
import oracle_lib as O
import outcome_model as M
import starts_batches as SB

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFF
SHARED_STARTS = (0, 4, 9, 13, 21, len(FB.custom_starts()) - 5)  # a handful of fide_replay_batches.custom_starts()
SHARED_CLOCKS = (0, 99, 140, 7, 149, 134)


def outcomes_list(out):
    return [(int(o["result"]), int(o["end_ply"]), int(o["repeats"]), int(o["halfmove"])) for o in out]


def assert_same_pos(got, want):
    bad = np.flatnonzero(~SB.same_pos(got, want).all(axis=1))
    assert len(bad) == 0, [(int(g), got[g], want[g]) for g in bad[:3]]


def tokens_of(engine, mv, start=None, halfmove=0):
    """The product's tokens of the accepted plies of a shared-start batch (NONE elsewhere)."""
    san = engine.replay_san(mv, start, halfmove)[1]
    tokens = np.full(mv.shape, dchess.SAN_TOKEN_NONE, np.uint32)
    for p, g in np.argwhere(san != 0xFF):
        tokens[p, g] = dchess.san_parse(dchess.san_format(int(mv[p, g]), int(san[p, g])))
    # a token that no longer fits, so that flagged words and first_bad occur
    tokens[mv.shape[0] // 2:, ::5] = np.roll(tokens[mv.shape[0] // 2:, ::5], 1, axis=0)
    return tokens


def same_tuple(got, want):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        if isinstance(b, dict):
            assert a == b, k
        else:
            assert a.dtype == b.dtype and a.shape == b.shape and (a == b).all(), k


# ------------------------------------------------- 1. against the shared-start calls
@pytest.fixture(scope="module")
def startpos_games():
    return O.fast_gen_games(2024, 0, 257, 40, 32, O.FIDE)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_null_starts_equal_the_shared_start_calls(engine, startpos_games, n):
    mv = np.ascontiguousarray(startpos_games[:, :n])
    same_tuple(engine.replay_outcome_starts(mv)[:5], engine.replay_outcome(mv))
    same_tuple(engine.replay_san_starts(mv)[:6], engine.replay_san(mv))
    tokens = tokens_of(engine, mv)
    got = engine.resolve_san_starts(tokens)
    same_tuple(got[:3], engine.resolve_san(tokens))
    assert int(got[2][dchess.SR_NOMATCH]) > 0 or n == 1
    # from the start position with nothing accepted the finals are the start position
    none = np.full((3, n), NONE, np.uint16)
    finals = engine.replay_outcome_starts(none)[5]
    assert_same_pos(finals, np.array([dchess.startpos()] * n, dchess.POS_DTYPE))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_one_start_repeated_equals_the_shared_start_calls(engine, n):
    for i, hm in zip(SHARED_STARTS, SHARED_CLOCKS):
        p = FB.custom_starts()[i][1]
        start = SB.dpos(p)
        mv = np.ascontiguousarray(np.tile(FB.games_from(i), (1, 5))[:, :n])
        starts = np.array([start] * n, dchess.POS_DTYPE)
        clocks = np.full(n, hm, np.uint16)
        a = engine.replay_outcome_starts(mv, starts, clocks)
        same_tuple(a[:5], engine.replay_outcome(mv, start, hm))
        b = engine.replay_san_starts(mv, starts, clocks)
        same_tuple(b[:6], engine.replay_san(mv, start, hm))
        assert_same_pos(a[5], b[6])
        tokens = tokens_of(engine, mv, start, hm)
        same_tuple(engine.resolve_san_starts(tokens, starts)[:3], engine.resolve_san(tokens, start))


# ------------------------------------------------------- 2. the mixed batch, the models
def check_replay(got, exp, with_san):
    if with_san:
        out, san, bm, dg, counts, st, finals = got
        bad = np.argwhere(san != exp.san)
        assert len(bad) == 0, [(int(p), int(g), int(san[p, g]), int(exp.san[p, g])) for p, g in bad[:5]]
    else:
        out, bm, dg, counts, st, finals = got
    wrong = [(g, a, b) for g, (a, b) in enumerate(zip(outcomes_list(out), exp.outcomes)) if a != b]
    assert not wrong, wrong[:5]
    assert (bm == exp.bitmap).all() and (dg == exp.digests).all()
    assert counts.tolist() == exp.counts
    assert st == exp.stats
    assert_same_pos(finals, exp.finals)


def test_mixed_batch_outcome(engine):
    b = SB.mixed()
    check_replay(engine.replay_outcome_starts(b.moves, b.dstarts, b.clocks), SB.mixed_expected(), False)


def test_mixed_batch_san(engine):
    b = SB.mixed()
    check_replay(engine.replay_san_starts(b.moves, b.dstarts, b.clocks), SB.mixed_expected(), True)


def test_mixed_batch_resolve(engine):
    b, r = SB.mixed(), SB.mixed_resolve()
    moves, first_bad, counts, finals = engine.resolve_san_starts(r.tokens, b.dstarts)
    bad = np.argwhere(moves != r.moves)
    assert len(bad) == 0, [(int(p), int(g), hex(int(moves[p, g])), hex(int(r.moves[p, g]))) for p, g in bad[:5]]
    assert (first_bad == r.first_bad).all() and counts.tolist() == r.counts.tolist()
    assert_same_pos(finals, r.finals)


# --------------------------------------------------------------- 3. chunk indexing
def test_chunks_index_by_game(engine):
    """257 games with 257 starts in chunks of 256: the second launch's only game is
    game 256 and reads starts[256] and its clock, writes finals[256]."""
    b = SB.distinct_starts()
    e = SB.Expected(b)
    hook = dchess.lib().dc_test_outcome_chunk_games
    hook.argtypes, hook.restype = [C.c_void_p, C.c_uint32], C.c_int
    engine.set_profiling(True)
    engine.reset_stats()
    assert hook(engine.ctx, 256) == 0
    try:
        got = engine.replay_outcome_starts(b.moves, b.dstarts, b.clocks)
        ks = engine.kernel_stats("replay_outcome_starts")
        got_san = engine.replay_san_starts(b.moves, b.dstarts, b.clocks)
        ks_san = engine.kernel_stats("replay_san_starts")
    finally:
        assert hook(engine.ctx, 177664) == 0
        engine.set_profiling(False)
    assert outcomes_list(got[0])[256] == e.outcomes[256] and got[2][256] == e.digests[256]
    assert_same_pos(got[5][256:], e.finals[256:])
    check_replay(got, e, False)
    check_replay(got_san, e, True)
    assert ks["launches"] == 2 and ks["units"] == e.stats["validated"]
    assert ks_san["launches"] == 2 and ks_san["units"] == e.stats["validated"]


# -------------------------------------------------- 4. clocks and repetition per lane
def test_shuffle_wave_clocks_per_lane(engine):
    b = SB.shuffle_wave()
    e = SB.Expected(b)
    check_replay(engine.replay_outcome_starts(b.moves, b.dstarts, b.clocks), e, False)
    check_replay(engine.replay_san_starts(b.moves, b.dstarts, b.clocks), e, True)
    # starts NULL with clocks alone: the same wave
    check_replay(engine.replay_outcome_starts(b.moves, None, b.clocks), e, False)


# ------------------------------------------------------------------ 5. permutation
def test_permuting_the_games_permutes_the_results(engine):
    b, r = SB.mixed(), SB.mixed_resolve()
    perm = np.random.default_rng(5).permutation(b.n)
    q = b.take(perm)
    out, san, bm, dg, counts, st, finals = engine.replay_san_starts(b.moves, b.dstarts, b.clocks)
    pout, psan, pbm, pdg, pcounts, pst, pfinals = engine.replay_san_starts(q.moves, q.dstarts, q.clocks)
    assert (pout == out[perm]).all() and (pdg == dg[perm]).all() and (psan == san[:, perm]).all()
    assert_same_pos(pfinals, finals[perm])
    assert (pcounts == counts).all() and pst == st
    oout, _, odg, ocounts, ost, ofinals = engine.replay_outcome_starts(q.moves, q.dstarts, q.clocks)
    assert (oout == out[perm]).all() and (odg == dg[perm]).all() and (ocounts == counts).all() and ost == st
    assert_same_pos(ofinals, finals[perm])
    moves, first_bad, rcounts, rfinals = engine.resolve_san_starts(r.tokens, b.dstarts)
    pmoves, pfirst, prcounts, prfinals = engine.resolve_san_starts(np.ascontiguousarray(r.tokens[:, perm]), q.dstarts)
    assert (pmoves == moves[:, perm]).all() and (pfirst == first_bad[perm]).all() and (prcounts == rcounts).all()
    assert_same_pos(prfinals, rfinals[perm])


# ----------------------------------------------------------------- 6. continuation
@pytest.mark.parametrize("k", [1, 11])
def test_continuation_from_finals(engine, k):
    """The first k plies, then the rest from finals and the outcomes' halfmove.
    Occurrences are counted from each call's start, so repeats (and with it a
    fivefold ending) are not carried: games the model ends by fivefold are left out."""
    b, e = SB.mixed(), SB.mixed_expected()
    whole = engine.replay_outcome_starts(b.moves, b.dstarts, b.clocks)
    head = engine.replay_outcome_starts(np.ascontiguousarray(b.moves[:k]), b.dstarts, b.clocks)
    tail = engine.replay_outcome_starts(np.ascontiguousarray(b.moves[k:]), head[5], head[0]["halfmove"])
    keep = np.array([o[0] != M.FIVEFOLD for o in e.outcomes])
    assert int(keep.sum()) >= b.n - 10
    assert (tail[0]["result"][keep] == whole[0]["result"][keep]).all()
    assert (tail[0]["halfmove"][keep] == whole[0]["halfmove"][keep]).all()
    assert (tail[2][keep] == whole[2][keep]).all()
    assert_same_pos(tail[5][keep], whole[5][keep])
    mask = np.zeros(whole[1].shape[1], np.uint64)
    for g in np.flatnonzero(keep):
        mask[g >> 6] |= np.uint64(1 << (int(g) & 63))
    assert ((np.concatenate([head[1], tail[1]]) & mask) == (whole[1] & mask)).all()


# --------------------------------------------------------------- 7. argument checks
def test_host_forms_check_their_arguments(engine):
    L = dchess.lib()
    n, n_plies = 3, 2
    mv = np.tile(np.array(M.line("e2e4 e7e5"), np.uint16)[:, None], (1, n))
    tokens = np.full((n_plies, n), dchess.san_parse("e4"), np.uint32)
    good = np.array([dchess.startpos()] * n, dchess.POS_DTYPE)
    stm2 = good.copy()
    stm2["stm"][1] = 2
    ok_clock, clock151 = np.array([0, 150, 3], np.uint16), np.array([0, 151, 3], np.uint16)
    fill = 0xAB

    def outputs():
        return [np.full(k, fill, np.uint8) for k in (8 * n, n_plies * n, 8 * n_plies, 8 * n, 8 * 7, 40, 40 * n)]

    for starts, clocks in ((stm2, ok_clock), (good, clock151), (stm2, None), (None, clock151)):
        for with_san in (False, True):
            out, san, bm, dg, counts, st, finals = outputs()
            p = lambda a: dchess._ptr(a)  # noqa: E731
            if with_san:
                r = L.dc_replay_san_starts(engine.ctx, p(starts), p(clocks), p(mv), n, n_plies, p(out), p(san), p(bm),
                                           p(dg), p(counts), C.cast(p(st), C.POINTER(dchess._Stats)), p(finals))
            else:
                r = L.dc_replay_outcome_starts(engine.ctx, p(starts), p(clocks), p(mv), n, n_plies, p(out), p(bm),
                                               p(dg), p(counts), C.cast(p(st), C.POINTER(dchess._Stats)), p(finals))
            assert r == dchess.EINVAL
            for a in (out, san, bm, dg, counts, st, finals):
                assert (a == fill).all()
    moves, fb, counts, finals = (np.full(k, fill, np.uint8) for k in (2 * n_plies * n, 4 * n, 8 * 5, 40 * n))
    r = L.dc_san_resolve_starts(engine.ctx, dchess._ptr(stm2), dchess._ptr(tokens), n, n_plies, dchess._ptr(moves),
                                dchess._ptr(fb), dchess._ptr(counts), dchess._ptr(finals))
    assert r == dchess.EINVAL
    for a in (moves, fb, counts, finals):
        assert (a == fill).all()
    with pytest.raises(dchess.DChessError) as err:
        engine.replay_outcome_starts(mv, stm2, ok_clock)
    assert err.value.status == dchess.EINVAL
    # the same arguments without the bad entry; finals NULL is accepted
    a = engine.replay_outcome_starts(mv, good, ok_clock, want_finals=False)
    assert a[5] is None and outcomes_list(a[0]) == [(0, 2, 1, 0), (M.SEVENTYFIVE, 0, 1, 150), (0, 2, 1, 0)]
    assert engine.replay_san_starts(mv, good, ok_clock, want_finals=False)[6] is None
    assert engine.resolve_san_starts(tokens, good, want_finals=False)[3] is None
    # no games: a successful no-op
    none = np.zeros((2, 0), np.uint16)
    out, bm, dg, counts, st, finals = engine.replay_outcome_starts(none, np.zeros(0, dchess.POS_DTYPE),
                                                                    np.zeros(0, np.uint16))
    assert len(out) == 0 and len(finals) == 0 and int(counts.sum()) == 0 and st["validated"] == 0
    assert len(engine.replay_san_starts(none, None, None)[0]) == 0
    moves, fb, counts, finals = engine.resolve_san_starts(np.zeros((2, 0), np.uint32))
    assert moves.shape == (2, 0) and len(finals) == 0 and int(counts.sum()) == 0
    # no plies: the finals are the starts
    b = SB.mixed()
    empty = np.zeros((0, b.n), np.uint16)
    assert_same_pos(engine.replay_outcome_starts(empty, b.dstarts, b.clocks)[5], b.dstarts)
    moves, fb, counts, finals = engine.resolve_san_starts(np.zeros((0, b.n), np.uint32), b.dstarts)
    assert_same_pos(finals, b.dstarts)
    assert not fb.any()


# ------------------------------------------------------------------ 8. _device forms
def test_device_forms(engine):
    b, r = SB.mixed(), SB.mixed_resolve()
    n, n_plies = b.n, b.moves.shape[0]
    words = (n + 63) // 64
    d_mv, d_st, d_hm = engine.alloc(b.moves.nbytes), engine.alloc(40 * n), engine.alloc(2 * n)
    d_out, d_san, d_bm, d_dg, d_fin = (engine.alloc(k) for k in (8 * n, n * n_plies, 8 * words * n_plies, 8 * n, 40 * n))
    d_mv.upload(b.moves)
    d_st.upload(b.dstarts)

    def fetch(with_san):
        got = [d_out.download(dchess.OUTCOME_DTYPE, n)]
        if with_san:
            got.append(d_san.download(np.uint8, n * n_plies).reshape(n_plies, n))
        return got + [d_bm.download(np.uint64, words * n_plies).reshape(n_plies, words), d_dg.download(np.uint64, n)]

    for clocks in (b.clocks, np.where(b.clocks == 150, 151, b.clocks).astype(np.uint16)):
        # on the device a clock above 150 behaves as 150
        assert (clocks != b.clocks).any() or clocks is b.clocks
        d_hm.upload(clocks)
        host = engine.replay_outcome_starts(b.moves, b.dstarts, b.clocks)
        counts, st = engine.replay_outcome_starts_device(d_mv, n, n_plies, d_out, d_bm, d_dg, d_st, d_hm, d_fin)
        same_tuple(fetch(False) + [counts, st, d_fin.download(dchess.POS_DTYPE, n)], host)
        host = engine.replay_san_starts(b.moves, b.dstarts, b.clocks)
        counts, st = engine.replay_san_starts_device(d_mv, n, n_plies, d_out, d_san, d_bm, d_dg, d_st, d_hm, d_fin)
        same_tuple(fetch(True) + [counts, st, d_fin.download(dchess.POS_DTYPE, n)], host)
    # everything optional left out
    counts, st = engine.replay_outcome_starts_device(d_mv, n, n_plies, d_out)
    same_tuple([counts, st], engine.replay_outcome(b.moves)[3:])
    d_tok, d_moves, d_fb = engine.alloc(r.tokens.nbytes), engine.alloc(2 * n * n_plies), engine.alloc(4 * n)
    d_tok.upload(r.tokens)
    counts = engine.resolve_san_starts_device(d_tok, n, n_plies, d_moves, d_fb, d_st, d_fin)
    host = engine.resolve_san_starts(r.tokens, b.dstarts)
    same_tuple([d_moves.download(np.uint16, n * n_plies).reshape(n_plies, n), d_fb.download(np.uint32, n), counts,
                d_fin.download(dchess.POS_DTYPE, n)], host)
    for d in (d_mv, d_st, d_hm, d_out, d_san, d_bm, d_dg, d_fin, d_tok, d_moves, d_fb):
        d.free()


# --------------------------------------------------------------- 9. tools/pgn_replay.py
class CountingEngine:
    """Passes every call on to the engine and counts the calls by name."""

    def __init__(self, engine):
        self.engine, self.calls = engine, {}

    def __getattr__(self, name):
        f = getattr(self.engine, name)

        def call(*a, **kw):
            self.calls[name] = self.calls.get(name, 0) + 1
            return f(*a, **kw)
        return call


def test_pgn_replay_one_batch_per_file(engine):
    spec = importlib.util.spec_from_file_location("pgn_replay", os.path.join(ROOT, "tools", "pgn_replay.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    b, e = SB.mixed(), SB.mixed_expected()
    token = {M.ONGOING: "*", M.WHITE_WINS: "1-0", M.BLACK_WINS: "0-1"}
    text = []
    for g in range(b.n):
        stm, fullmove = b.starts[g].stm, 10 + g
        fen = dchess.pos_to_fen(b.dstarts[g], int(b.clocks[g]), fullmove)
        result = e.outcomes[g][0]
        text.append('[Result "%s"]\n[SetUp "1"]\n[FEN "%s"]\n\n%s\n' % (
            token.get(result, "1/2-1/2"), fen,
            dchess.pgn_movetext(b.moves[:, g], e.san[:, g], result, fullmove, stm)))
    assert len({t.split("\n")[2] for t in text}) >= 100  # many distinct FEN tags
    games, broken = tool.load("\n".join(text))
    assert len(games) == b.n and not broken
    counting = CountingEngine(engine)
    done = tool.replay(counting, games)
    assert counting.calls == {"resolve_san_starts": 1, "replay_san_starts": 1}
    for g in range(b.n):
        moves, first_bad, out, fen = done[g]
        played = b.moves[:, g][np.array(e.games[g]["accept"])]
        assert moves.tolist() == played.tolist(), g
        assert first_bad >= len(played)  # no flagged word: the batch's n_plies
        result, end_ply, repeats, halfmove = e.outcomes[g]
        assert (int(out["result"]), int(out["repeats"]), int(out["halfmove"])) == (result, repeats, halfmove), g
        if result != M.ONGOING:
            assert int(out["end_ply"]) == len(played)
        want = dchess.pos_to_fen(e.finals[g], halfmove, 10 + g + (b.starts[g].stm + len(played)) // 2)
        assert fen == want, g
