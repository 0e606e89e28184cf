"""GPU tests of dc_san_resolve against its model (tests/san_resolve_model.py,
pinned by tests/test_san_resolve_model.py): the constructed positions, the
round trip move -> SAN text -> token -> move over the seeded batches and back
through dc_replay_san, the way through PGN text, corrupted tokens (where the
games diverge from what was played and only the model knows the answer), the
batch shapes at which waves and blocks change, a Black-to-move start, empty
batches, the host and device forms, the argument checks and the timing name.
Everything is integer or text and compared exactly."""
import numpy as np
import pytest

import dchess
import oracle_lib as O
import san_model as S
import san_resolve_model as R
from test_san_resolve_model import CASES, tokens_of

pytestmark = pytest.mark.gpu

NONE = dchess.SAN_TOKEN_NONE
BLACK_FEN = "r3k2r/pp3ppp/2n5/8/8/2N5/PP3PPP/R3K2R b KQkq - 147 60"


@pytest.fixture(scope="module")
def seeded():
    """noise -> (moves, SAN bytes, accepted mask, tokens made by the product:
    san_parse(san_format(move, byte)) per distinct (move, byte), NONE elsewhere)."""
    ref = {}
    for noise in (0, 32):
        mv, san, _ = R.seeded(noise)
        ok = san != S.NONE
        key = mv.astype(np.uint32) | (san.astype(np.uint32) << 16)
        uniq, inv = np.unique(key[ok], return_inverse=True)
        toks = np.array([dchess.san_parse(dchess.san_format(int(k) & 0xFFFF, int(k) >> 16)) for k in uniq], np.uint32)
        tokens = np.full(mv.shape, NONE, np.uint32)
        tokens[ok] = toks[inv]
        ref[noise] = (mv, san, ok, tokens)
    return ref


def same(got, want):
    moves, first_bad, counts = got
    wmoves, wfirst, wcounts = want
    bad = np.argwhere(moves != wmoves)
    assert len(bad) == 0, [(int(p), int(g), hex(int(moves[p, g])), hex(int(wmoves[p, g]))) for p, g in bad[:5]]
    assert (first_bad == wfirst).all() and counts.tolist() == wcounts.tolist()


def test_constructed_positions(engine):
    """The positions of test_san_resolve_model.py, batched per start FEN: the words
    pinned there, and the model's words, first_bad and counts."""
    groups = {}
    for name, fen, items, want in CASES:
        groups.setdefault(fen, []).append((name, tokens_of(items), want))
    for fen, cases in groups.items():
        start, ostart = (dchess.pos_from_fen(fen), O.Pos.from_fen(fen)) if fen else (None, None)
        tokens = R.pad_tokens([c[1] for c in cases])
        got = engine.resolve_san(tokens, start)
        for g, (name, _, want) in enumerate(cases):
            assert [hex(w) for w in got[0][:len(want), g]] == [hex(w) for w in want], name
            assert (got[0][len(want):, g] == dchess.MOVE_NONE).all(), name
        same(got, R.walk_batch(tokens, ostart))


@pytest.mark.parametrize("noise", [0, 32])
def test_round_trip(engine, seeded, noise):
    """Every accepted ply resolves to the move that was played, every other ply to
    MOVE_NONE; replaying the resolved moves gives what replaying the originals gave.
    The replay's `validated` and `rejected` count the originals' rejected plies, which
    the resolved array holds as MOVE_NONE: there validated = accepted and rejected = 0
    (with no rejected ply, as in the noise-0 batch, that is equality of all five)."""
    mv, wsan, ok, tokens = seeded[noise]
    moves, first_bad, counts = engine.resolve_san(tokens)
    want = np.where(ok, mv, dchess.MOVE_NONE).astype(np.uint16)
    bad = np.argwhere(moves != want)
    assert len(bad) == 0, [(int(p), int(g), hex(int(moves[p, g])), hex(int(want[p, g]))) for p, g in bad[:5]]
    assert (first_bad == mv.shape[0]).all()
    assert counts.tolist() == [int(ok.sum()), int(ok.sum()), 0, 0, 0]
    out, san, bm, dg, gcounts, st = engine.replay_san(mv)
    rout, rsan, rbm, rdg, rcounts, rst = engine.replay_san(moves)
    assert (san == wsan).all()
    assert (rout == out).all() and (rsan == san).all() and (rbm == bm).all() and (rdg == dg).all()
    assert (rcounts == gcounts).all()
    assert rst == dict(st, validated=st["accepted"], rejected=0)
    if noise == 0:
        assert rst == st


def test_via_text(engine, seeded):
    """pgn_movetext -> pgn_parse_movetext -> resolve_san for a handful of games: the
    accepted moves, in order."""
    mv, _, ok, _ = seeded[32]
    games = [0, 1, 63, 64, 200, 256]
    sub = np.ascontiguousarray(mv[:, games])
    out, san = engine.replay_san(sub)[:2]
    columns = []
    for k in range(len(games)):
        text = dchess.pgn_movetext(sub[:, k], san[:, k], int(out[k]["result"]))
        tokens, result, fullmove, stm, used = dchess.pgn_parse_movetext(text)
        assert (fullmove, stm, used) == (1, 0, len(text))
        assert result == min(int(out[k]["result"]), dchess.PGN_DRAW)
        columns.append(tokens)
    moves, first_bad, counts = engine.resolve_san(R.pad_tokens(columns))
    for k, g in enumerate(games):
        played = mv[:, g][ok[:, g]]
        assert len(played) == len(columns[k]) > 0
        assert moves[:len(played), k].tolist() == played.tolist(), g
        assert (moves[len(played):, k] == dchess.MOVE_NONE).all() and first_bad[k] == moves.shape[0]
    assert counts.tolist() == [sum(map(len, columns)), sum(map(len, columns)), 0, 0, 0]


def corrupt(tokens, seed=2024):
    """A seeded tenth of the tokens overwritten: every needed hint dropped and every
    promotion dropped (both are rare), and over the rest of the tenth a wrong file
    hint, a random 32-bit word or NONE."""
    rng = np.random.default_rng(seed)
    out = tokens.copy()
    flat = out.reshape(-1)
    live = np.flatnonzero(flat != NONE)
    t = flat[live]
    castle = t & (R.OO | R.OOO) != 0
    piece = ((t >> 6) & 7 != 0) & ~castle
    hinted = piece & (t & (R.FILE_GIVEN | R.RANK_GIVEN) != 0)
    promo = ((t >> 9) & 7 != 0) & ~castle
    n = len(live) // 10
    rare = np.flatnonzero(hinted | promo)
    assert 0 < len(rare) < n
    rest = rng.choice(np.flatnonzero(~(hinted | promo)), n - len(rare), replace=False)
    flat[live[hinted]] &= ~np.uint32(R.FILE_GIVEN | R.RANK_GIVEN | (7 << 13) | (7 << 17))
    flat[live[promo]] &= ~np.uint32(7 << 9)
    how = rng.integers(0, 3, len(rest))
    words = rng.integers(0, 1 << 32, len(rest), dtype=np.uint64).astype(np.uint32)
    shift = rng.integers(1, 8, len(rest)).astype(np.uint32)
    for i, h, w, s in zip(live[rest].tolist(), how.tolist(), words.tolist(), shift.tolist()):
        if h == 0:  # a file that is not the origin's (for a castle: a field that may not be there)
            cur = int(flat[i])
            file = (((cur >> 13) & 7 if cur & R.FILE_GIVEN else cur & 7) + s) & 7
            flat[i] = (cur & ~(7 << 13)) | R.FILE_GIVEN | (file << 13)
        else:
            flat[i] = w if h == 1 else NONE
    return out


def test_corrupted_tokens(engine, seeded):
    """After a bad token the game is no longer the one that was played: the model is
    the reference at every ply, none excluded."""
    tokens = corrupt(seeded[0][3])
    assert int((tokens != seeded[0][3]).sum()) >= int((seeded[0][3] != NONE).sum()) // 11
    want = R.walk_batch(tokens)
    got = engine.resolve_san(tokens)
    same(got, want)
    for word in (dchess.MOVE_NOMATCH, dchess.MOVE_AMBIGUOUS, dchess.MOVE_MALFORMED, dchess.MOVE_NONE):
        assert (got[0] == word).any(), hex(word)
    assert all(int(c) > 0 for c in got[2])
    assert (got[1] < tokens.shape[0]).any()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257])
def test_batch_shapes(engine, seeded, n):
    mv, _, ok, tokens = seeded[32]
    moves, first_bad, counts = engine.resolve_san(np.ascontiguousarray(tokens[:, :n]))
    assert (moves == np.where(ok, mv, dchess.MOVE_NONE)[:, :n]).all()
    assert (first_bad == mv.shape[0]).all() and counts.tolist() == [int(ok[:, :n].sum())] * 2 + [0, 0, 0]


def test_black_to_move_start(engine):
    lines = [["O-O", "O-O-O", "Rad8", "Rxd8+", "Rxd8", "Nd5"], ["O-O-O", "O-O", "Rd1", "Rxd1", "Rd8", "Nb4"],
             ["Nb4", "Nb5", "Nd3+", "Ke2", "Nxb2", "Nc7+", "Kd7", "Nxa8"], ["e5"], ["Ke7", "Ke2", "Kf1"]]
    tokens = R.pad_tokens([[dchess.san_parse(s) for s in l] for l in lines])
    want = R.walk_batch(tokens, O.Pos.from_fen(BLACK_FEN))
    assert want[2][dchess.SR_RESOLVED] >= 15 and want[2][dchess.SR_NOMATCH] >= 2 and want[2][dchess.SR_AMBIGUOUS] >= 1
    same(engine.resolve_san(tokens, dchess.pos_from_fen(BLACK_FEN)), want)


def test_no_plies_and_no_games(engine):
    moves, first_bad, counts = engine.resolve_san(np.zeros((0, 65), np.uint32))
    assert moves.shape == (0, 65) and first_bad.tolist() == [0] * 65 and counts.tolist() == [0] * 5
    moves, first_bad, counts = engine.resolve_san(np.zeros((3, 0), np.uint32))
    assert moves.shape == (3, 0) and len(first_bad) == 0 and counts.tolist() == [0] * 5
    d_fb = engine.alloc(4 * 65)
    d_fb.upload(np.full(65, 7, np.uint32))
    counts = engine.resolve_san_device(None, 65, 0, None, d_fb)
    assert d_fb.download(np.uint32, 65).tolist() == [0] * 65 and counts.tolist() == [0] * 5
    assert engine.resolve_san_device(None, 0, 3, None).tolist() == [0] * 5


def test_host_and_device_forms_agree(engine, seeded):
    tokens = np.ascontiguousarray(corrupt(seeded[32][3], seed=7)[:, :65])
    n_plies, n = tokens.shape
    moves, first_bad, counts = engine.resolve_san(tokens)
    d_tok, d_mv, d_fb = engine.alloc(tokens.nbytes), engine.alloc(2 * n * n_plies), engine.alloc(4 * n)
    d_tok.upload(tokens)
    dcounts = engine.resolve_san_device(d_tok, n, n_plies, d_mv, d_fb)
    assert (d_mv.download(np.uint16, n * n_plies).reshape(n_plies, n) == moves).all()
    assert (d_fb.download(np.uint32, n) == first_bad).all() and (dcounts == counts).all()
    assert (first_bad < n_plies).any()
    # first_bad and counts are optional, the moves do not depend on them
    d_mv.upload(np.zeros(n * n_plies, np.uint16))
    assert engine.resolve_san_device(d_tok, n, n_plies, d_mv, None, want_counts=False) is None
    assert (d_mv.download(np.uint16, n * n_plies).reshape(n_plies, n) == moves).all()
    moves2, fb2, counts2 = engine.resolve_san(tokens, want_first_bad=False, want_counts=False)
    assert fb2 is None and counts2 is None and (moves2 == moves).all()
    # the resolved array goes to the replay as it is: a flagged word is a rejected ply
    st = engine.replay_san(moves)[5]
    assert st["accepted"] <= int(counts[dchess.SR_RESOLVED]) and st["rejected"] > 0


def test_null_pointers_and_turn_are_einval(engine):
    L = dchess.lib()
    tok = np.array([dchess.san_parse("e4")], np.uint32)
    mv = np.full(1, 0x1234, np.uint16)
    fb = np.full(1, 77, np.uint32)
    counts = np.full(dchess.SR_COUNT, 77, np.uint64)
    t, m, f, c = dchess._ptr(tok), dchess._ptr(mv), dchess._ptr(fb), dchess._ptr(counts)
    bad = np.array([dchess.startpos()], dchess.POS_DTYPE)
    bad["stm"] = 2
    d_tok, d_mv = engine.alloc(4), engine.alloc(2)
    d_tok.upload(tok)
    d_mv.upload(mv)
    assert L.dc_san_resolve(engine.ctx, None, None, 1, 1, m, f, c) == dchess.EINVAL
    assert L.dc_san_resolve(engine.ctx, None, t, 1, 1, None, f, c) == dchess.EINVAL
    assert L.dc_san_resolve(engine.ctx, dchess._ptr(bad), t, 1, 1, m, f, c) == dchess.EINVAL
    assert L.dc_san_resolve(None, None, t, 1, 1, m, f, c) == dchess.EINVAL
    assert L.dc_san_resolve_device(engine.ctx, None, None, 1, 1, d_mv.ptr, None, c) == dchess.EINVAL
    assert L.dc_san_resolve_device(engine.ctx, None, d_tok.ptr, 1, 1, None, None, c) == dchess.EINVAL
    assert L.dc_san_resolve_device(engine.ctx, dchess._ptr(bad), d_tok.ptr, 1, 1, d_mv.ptr, None, c) == dchess.EINVAL
    # nothing was written
    assert mv[0] == 0x1234 and fb[0] == 77 and (counts == 77).all()
    assert d_mv.download(np.uint16, 1)[0] == 0x1234
    # NULL pointers are fine where there is nothing to read or write
    assert L.dc_san_resolve(engine.ctx, None, None, 0, 5, None, None, None) == 0
    assert L.dc_san_resolve(engine.ctx, None, None, 5, 0, None, None, None) == 0
    assert L.dc_san_resolve(engine.ctx, None, t, 1, 1, m, None, None) == 0 and mv[0] == (12 | (28 << 6))


def test_timing_name(engine, seeded):
    tokens = np.ascontiguousarray(seeded[0][3][:, :65])
    engine.set_profiling(True)
    engine.reset_stats()
    try:
        counts = engine.resolve_san(tokens)[2]
        ks = engine.kernel_stats("san_resolve")
    finally:
        engine.set_profiling(False)
    assert ks["launches"] == 1 and ks["units"] == int(counts[dchess.SR_TOKENS]) > 0 and ks["total_ms"] > 0
