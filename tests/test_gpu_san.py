"""GPU tests of dc_replay_san against the SAN model (tests/san_model.py, pinned
by tests/test_san_model.py): the pinned positions and games, seeded games in
which every class of SAN byte occurs, the batch shapes at which the kernel's
waves, blocks and chunks change, the host and device forms, a Black-to-move
start with a running clock, terminal starts and the timing name.  Everything
besides the SAN bytes must equal dc_replay_outcome's on the same input.
Everything is integer or text and compared exactly."""
import ctypes as C

import numpy as np
import pytest

import dchess
import oracle_lib as O
import outcome_model as M
import san_model as S
from test_gpu_outcome import MATE_FEN, STALE_FEN, DEAD_FEN, outcomes_list, pad_games
from test_outcome_model import PINNED
from test_san_model import LINES, MOVETEXT

pytestmark = pytest.mark.gpu

NONE = 0xFFFF


@pytest.fixture(scope="module")
def seeded():
    """noise -> (moves, model SAN bytes [n_plies, n_games], [(result, end_ply)]): the
    257-game batches of tests/test_gpu_outcome.py, annotated once."""
    ref = {}
    for noise in (0, 32):
        mv = O.fast_gen_games(2024, 0, 257, 600, noise, O.FIDE)
        ref[noise] = (mv,) + S.annotate_batch(mv)
    return ref


def same_as_outcome(engine, mv, got, start=None, hm=0):
    """outcomes, bitmap, digests, counts and stats of a replay_san result equal replay_outcome's."""
    out, _, bm, dg, counts, st = got
    rout, rbm, rdg, rcounts, rst = engine.replay_outcome(mv, start, hm)
    assert (out == rout).all() and (bm == rbm).all() and (dg == rdg).all()
    assert (counts == rcounts).all() and st == rst


def classes(mv, san):
    """How often each class of SAN byte occurs in a batch."""
    ok = san != S.NONE
    kind, flags = san & 7, san & (S.FILE | S.RANK)
    files = (mv & 7).astype(np.int32) - ((mv >> 6) & 7).astype(np.int32)
    castle = ok & (kind == M.K) & (np.abs(files) == 2)
    return {"accepted": int(ok.sum()), "capture": int((ok & (san & S.CAPTURE != 0)).sum()),
            "file": int((ok & (flags == S.FILE)).sum()), "rank": int((ok & (flags == S.RANK)).sum()),
            "check": int((ok & (san & S.CHECK != 0)).sum()), "mate": int((ok & (san & S.MATE != 0)).sum()),
            "promotion": int((ok & ((mv >> 12) & 7 != 0)).sum()), "O-O": int((castle & (files == -2)).sum()),
            "O-O-O": int((castle & (files == 2)).sum())}


def test_pinned_positions(engine):
    """The lines of test_san_model.py, batched per start position: bytes and strings."""
    groups = {}
    for fen, moves, want in LINES:
        groups.setdefault(fen, []).append((M.line(moves), want))
    for fen, lines in groups.items():
        start, ostart = (dchess.pos_from_fen(fen), O.Pos.from_fen(fen)) if fen else (None, None)
        mv = pad_games([l[0] for l in lines])
        got = engine.replay_san(mv, start)
        san = got[1]
        for g, (line, want) in enumerate(lines):
            r = S.annotate(mv[:, g], ostart)
            assert san[:, g].tolist() == r["san"], (fen, g)
            toks = [dchess.san_format(int(m), int(b)) for m, b in zip(mv[:, g], san[:, g]) if b != S.NONE]
            assert " ".join(toks) == want, (fen, g)
        same_as_outcome(engine, mv, got, start)


def test_pinned_games(engine):
    """The games of test_outcome_model.py: bytes, movetext, 0xFF exactly where no move
    was made, MATE exactly on the last move of a won game."""
    groups = {}
    for name, fen, hm, moves, want in PINNED:
        groups.setdefault((fen, hm), []).append((name, M.line(moves), want))
    for (fen, hm), games in groups.items():
        start, ostart = (dchess.pos_from_fen(fen), O.Pos.from_fen(fen)) if fen else (None, None)
        mv = pad_games([g[1] for g in games])
        got = engine.replay_san(mv, start, hm)
        out, san, bm = got[0], got[1], got[2]
        assert outcomes_list(out) == [g[2] for g in games], (fen, hm)
        for g, (name, line, want) in enumerate(games):
            r = S.annotate(mv[:, g], ostart, hm)
            assert san[:, g].tolist() == r["san"], name
            end = want[1]
            for p in range(mv.shape[0]):
                accepted = (int(bm[p, g >> 6]) >> (g & 63)) & 1
                assert (san[p, g] == S.NONE) == (not accepted), (name, p)
                assert p < end or san[p, g] == S.NONE, (name, p)
            mates = [p for p in range(mv.shape[0]) if san[p, g] != S.NONE and san[p, g] & S.MATE]
            won = want[0] in (M.WHITE_WINS, M.BLACK_WINS)
            assert mates == ([end - 1] if won else []), name
            text = dchess.pgn_movetext(mv[:, g], san[:, g], int(out[g]["result"]), 1, ostart.stm if ostart else 0)
            assert text == MOVETEXT[name], name
        same_as_outcome(engine, mv, got, start, hm)


@pytest.mark.parametrize("noise", [0, 32])
def test_seeded_games(engine, seeded, noise):
    mv, wsan, ends = seeded[noise]
    # the batch must hold every class of byte (FILE|RANK together: the pinned Qh4e1)
    cl = classes(mv, wsan)
    print(noise, cl)
    for k, v in cl.items():
        assert v >= 1, (k, cl)
    got = engine.replay_san(mv)
    out, san = got[0], got[1]
    bad = np.argwhere(san != wsan)
    assert len(bad) == 0, [(int(p), int(g), hex(int(mv[p, g])), int(san[p, g]), int(wsan[p, g])) for p, g in bad[:5]]
    assert [(int(o["result"]), int(o["end_ply"])) for o in out] == ends
    for g, (result, end) in enumerate(ends):
        assert (san[end:, g] == S.NONE).all()
        won = result in (M.WHITE_WINS, M.BLACK_WINS)
        col = san[:, g]
        mates = np.flatnonzero((col != S.NONE) & (col & S.MATE != 0)).tolist()
        assert mates == ([end - 1] if won else []), g
    same_as_outcome(engine, mv, got)
    # one game as text, through the product's formatter and the model's
    g = next(g for g, e in enumerate(ends) if e[0] in (M.WHITE_WINS, M.BLACK_WINS))
    assert dchess.pgn_movetext(mv[:, g], san[:, g], ends[g][0]) == S.movetext(mv[:, g], wsan[:, g], ends[g][0])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257])
def test_batch_shapes(engine, seeded, n):
    mv, wsan, ends = seeded[32]
    sub = np.ascontiguousarray(mv[:, :n])
    got = engine.replay_san(sub)
    assert (got[1] == wsan[:, :n]).all()
    assert [(int(o["result"]), int(o["end_ply"])) for o in got[0]] == ends[:n]
    same_as_outcome(engine, sub, got)


def test_chunks_share_the_history(engine, seeded):
    """257 games in chunks of 256: two launches, one history buffer, same bytes;
    the timing name reports the launches and the moves consumed."""
    mv, wsan, ends = seeded[32]
    hook = dchess.lib().dc_test_outcome_chunk_games
    hook.argtypes, hook.restype = [C.c_void_p, C.c_uint32], C.c_int
    engine.set_profiling(True)
    engine.reset_stats()
    assert hook(engine.ctx, 256) == 0
    try:
        got = engine.replay_san(mv)
        ks, ko = engine.kernel_stats("replay_san"), engine.kernel_stats("replay_outcome")
    finally:
        assert hook(engine.ctx, 177664) == 0
        engine.set_profiling(False)
    assert (got[1] == wsan).all()
    assert [(int(o["result"]), int(o["end_ply"])) for o in got[0]] == ends
    assert ks["launches"] == 2 and ks["units"] == got[5]["validated"] and ks["total_ms"] > 0
    assert ko["launches"] == 0
    same_as_outcome(engine, mv, got)


def test_timing_name(engine, seeded):
    mv = np.ascontiguousarray(seeded[0][0][:, :65])
    engine.set_profiling(True)
    engine.reset_stats()
    try:
        st = engine.replay_san(mv)[5]
        ks = engine.kernel_stats("replay_san")
    finally:
        engine.set_profiling(False)
    assert ks["launches"] == 1 and ks["units"] == st["validated"] > 0


def test_host_and_device_forms_agree(engine, seeded):
    mv = np.ascontiguousarray(seeded[32][0][:, :65])
    n_plies, n = mv.shape
    words = (n + 63) // 64
    out, san, bm, dg, counts, st = engine.replay_san(mv)
    d_mv, d_out, d_san = engine.alloc(mv.nbytes), engine.alloc(8 * n), engine.alloc(n * n_plies)
    d_bm, d_dg = engine.alloc(8 * words * n_plies), engine.alloc(8 * n)
    d_mv.upload(mv)
    dcounts, dst = engine.replay_san_device(d_mv, n, n_plies, d_out, d_san, d_bm, d_dg)
    assert (d_out.download(dchess.OUTCOME_DTYPE, n) == out).all()
    assert (d_san.download(np.uint8, n * n_plies).reshape(n_plies, n) == san).all()
    assert (d_bm.download(np.uint64, words * n_plies).reshape(n_plies, words) == bm).all()
    assert (d_dg.download(np.uint64, n) == dg).all()
    assert (dcounts == counts).all() and dst == st
    # bitmap and digests are optional, the bytes do not depend on them
    d_san.upload(np.zeros(n * n_plies, np.uint8))
    dcounts, dst = engine.replay_san_device(d_mv, n, n_plies, d_out, d_san)
    assert (dcounts == counts).all() and dst == st
    assert (d_san.download(np.uint8, n * n_plies).reshape(n_plies, n) == san).all()
    out2, san2, bm2, dg2, _, _ = engine.replay_san(mv, want_bitmap=False, want_digests=False)
    assert bm2 is None and dg2 is None and (san2 == san).all() and (out2 == out).all()


def test_black_to_move_with_a_running_clock(engine):
    """A non-start FEN, Black to move, half-move clock 147: the third reversible
    move reaches 150, the fourth belongs to no game."""
    fen = "r3k2r/pp3ppp/2n5/8/8/2N5/PP3PPP/R3K2R b KQkq - 147 60"
    hm, fm = dchess.fen_clocks(fen)
    lines = [M.line("e8g8 e1c1 a8d8 d1d8"), M.line("e8c8 e1g1 d8d1 f1d1"), M.line("c6b4 c3b5 b4d3 e1e2 d3b2")]
    mv = pad_games(lines)
    start, ostart = dchess.pos_from_fen(fen), O.Pos.from_fen(fen)
    got = engine.replay_san(mv, start, hm)
    out, san = got[0], got[1]
    want = [S.annotate(mv[:, g], ostart, hm) for g in range(3)]
    for g, r in enumerate(want):
        assert san[:, g].tolist() == r["san"], g
        assert (int(out[g]["result"]), int(out[g]["end_ply"])) == (r["result"], r["end_ply"])
    assert [r["end_ply"] for r in want] == [3, 3, 3]
    texts = [dchess.pgn_movetext(mv[:, g], san[:, g], int(out[g]["result"]), fm, 1) for g in range(3)]
    assert texts == ["60... O-O 61. O-O-O Rad8 1/2-1/2", "60... O-O-O 61. O-O Rd1 1/2-1/2",
                     "60... Nb4 61. Nb5 Nd3+ 1/2-1/2"]
    assert texts == [S.movetext(mv[:, g], want[g]["san"], want[g]["result"], fm, 1) for g in range(3)]
    assert dchess.pos_to_fen(start, hm, fm) == fen
    same_as_outcome(engine, mv, got, start, hm)


@pytest.mark.parametrize("fen,result", [(MATE_FEN, M.BLACK_WINS), (STALE_FEN, M.STALEMATE), (DEAD_FEN, M.DEAD)])
def test_terminal_start(engine, fen, result):
    hm = dchess.fen_clocks(fen)[0]
    mv = np.tile(np.array(M.line("e1e2 e8e7 a2a3 h8g8"), np.uint16)[:, None], (1, 3))
    got = engine.replay_san(mv, dchess.pos_from_fen(fen), hm)
    out, san = got[0], got[1]
    assert outcomes_list(out) == [(result, 0, 1, hm)] * 3
    assert (san == S.NONE).all()
    assert dchess.pgn_movetext(mv[:, 0], san[:, 0], int(out[0]["result"])) == S.RESULT_TOKEN[result]
    same_as_outcome(engine, mv, got, dchess.pos_from_fen(fen), hm)


def test_no_plies_and_no_games(engine):
    out, san, bm, dg, counts, st = engine.replay_san(np.zeros((0, 65), np.uint16), start_halfmove=7)
    assert outcomes_list(out) == [(dchess.GO_ONGOING, 0, 1, 7)] * 65 and san.shape == (0, 65)
    assert counts.tolist() == [65, 0, 0, 0, 0, 0, 0] and st["validated"] == 0
    out, san, _, _, counts, _ = engine.replay_san(np.zeros((3, 0), np.uint16))
    assert len(out) == 0 and san.shape == (3, 0) and int(counts.sum()) == 0


def test_null_pointers_and_clock_are_einval(engine):
    L = dchess.lib()
    out = np.zeros(1, dchess.OUTCOME_DTYPE)
    mv = np.array([M.mv("e2e4")], np.uint16)
    san = np.zeros(1, np.uint8)
    o, m, s = dchess._ptr(out), dchess._ptr(mv), dchess._ptr(san)
    for fn in (L.dc_replay_san, L.dc_replay_san_device):
        assert fn(engine.ctx, None, 0, None, 1, 1, o, s, None, None, None, None) == dchess.EINVAL
        assert fn(engine.ctx, None, 0, m, 1, 1, None, s, None, None, None, None) == dchess.EINVAL
        assert fn(engine.ctx, None, 0, m, 1, 1, o, None, None, None, None, None) == dchess.EINVAL
    with pytest.raises(dchess.DChessError) as e:
        engine.replay_san(mv.reshape(1, 1), start_halfmove=151)
    assert e.value.status == dchess.EINVAL
    d_mv, d_out, d_san = engine.alloc(2), engine.alloc(8), engine.alloc(1)
    d_mv.upload(mv)
    with pytest.raises(dchess.DChessError) as e:
        engine.replay_san_device(d_mv, 1, 1, d_out, d_san, start_halfmove=151)
    assert e.value.status == dchess.EINVAL
    assert san[0] == 0  # nothing was written
