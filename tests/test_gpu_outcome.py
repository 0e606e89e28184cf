"""GPU tests of dc_replay_outcome against the adjudication model
(tests/outcome_model.py): the pinned games of test_outcome_model.py, seeded
games that reach every result but fivefold, the batch shapes at which the
kernel's waves, blocks and chunks change, terminal start positions, and the
host and device forms.  Everything is integer and compared exactly.

The kernel keeps full position keys, not hashes, so there is no hash hook and
no truncated-hash rerun; the chunk hook (dc_test_outcome_chunk_games) covers
the path that replaces it: several launches sharing one history buffer."""
import ctypes as C

import numpy as np
import pytest

import dchess
import oracle_lib as O
import outcome_model as M
from test_outcome_model import PINNED

pytestmark = pytest.mark.gpu

NONE = 0xFFFF
MATE_FEN = "rnb1kbnr/pppp1ppp/8/4p3/6Pq/5P2/PPPPP2P/RNBQKBNR w KQkq - 1 3"
STALE_FEN = "7k/5Q2/6K1/8/8/8/8/8 b - - 0 1"
DEAD_FEN = "4k3/8/8/8/8/8/8/4K3 w - - 0 1"


def outcomes_list(out):
    return [(int(o["result"]), int(o["end_ply"]), int(o["repeats"]), int(o["halfmove"])) for o in out]


def pad_games(lines):
    n = max(len(m) for m in lines)
    mv = np.full((n, len(lines)), NONE, np.uint16)
    for g, m in enumerate(lines):
        mv[:len(m), g] = m
    return mv


def bit(bitmap, ply, g):
    return (int(bitmap[ply, g >> 6]) >> (g & 63)) & 1


@pytest.fixture(scope="module")
def seeded():
    """noise -> (moves, model result).  Noise 32 holds 257 games for the shape
    tests: the 256 of test_seeded_games and one more (a game depends on its id only)."""
    ref = {}
    for noise, n in ((0, 256), (32, 257)):
        mv = O.fast_gen_games(2024, 0, n, 600, noise, O.FIDE)
        ref[noise] = (mv, M.adjudicate_batch(mv))
    return ref


def test_pinned_games(engine):
    # one call per start position and clock: the five startpos games share a batch
    groups = {}
    for name, fen, hm, moves, want in PINNED:
        groups.setdefault((fen, hm), []).append((M.line(moves), want))
    assert max(len(v) for v in groups.values()) == 5
    for (fen, hm), games in groups.items():
        start = dchess.pos_from_fen(fen) if fen else None
        mv = pad_games([g[0] for g in games])
        out, bm, dg, counts, st = engine.replay_outcome(mv, start, hm)
        assert outcomes_list(out) == [g[1] for g in games], (fen, hm)
        assert counts.tolist() == [sum(1 for g in games if g[1][0] == k) for k in range(dchess.GO_COUNT)]
        cut = mv.copy()
        for g, (_, want) in enumerate(games):
            cut[want[1]:, g] = NONE
            assert not any(bit(bm, p, g) for p in range(want[1], mv.shape[0])), (fen, g)
        rbm, rdg, rst = engine.replay(cut, dchess.RULES_FIDE, start)
        assert (dg == rdg).all() and (bm == rbm).all()
        assert st == rst


@pytest.mark.parametrize("noise", [0, 32])
def test_seeded_games(engine, seeded, noise):
    mv, (want, wbm, wcounts, wst, wdg) = seeded[noise]
    mv, want, wbm, wdg = mv[:, :256], want[:256], wbm[:, :4], wdg[:256]
    if noise == 32:  # the model's totals hold game 256 too: take it out
        extra = M.adjudicate(seeded[32][0][:, 256])
        wcounts = list(wcounts)
        wcounts[extra["result"]] -= 1
        wst = {"validated": wst["validated"] - extra["validated"], "accepted": wst["accepted"] - extra["accepted"]}
        wst["rejected"] = wst["validated"] - wst["accepted"]
    # the batch must exercise every result but fivefold (covered by the pinned games)
    print(noise, wcounts, wst)
    for k in range(dchess.GO_COUNT):
        if k == dchess.GO_FIVEFOLD:
            continue
        assert wcounts[k] >= (5 if k == dchess.GO_ONGOING else 10), (k, wcounts)
    out, bm, dg, counts, st = engine.replay_outcome(mv)
    assert outcomes_list(out) == want
    assert (bm == wbm).all()
    assert counts.tolist() == wcounts
    assert {k: st[k] for k in ("validated", "accepted", "rejected")} == wst
    assert (dg == wdg).all()
    assert st["digest_sum"] == int(wdg.sum(dtype=np.uint64)) and st["digest_xor"] == int(np.bitwise_xor.reduce(wdg))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_shapes(engine, seeded, n):
    mv, (want, wbm, _, _, wdg) = seeded[32]
    sub = np.ascontiguousarray(mv[:, :n])
    out, bm, dg, counts, st = engine.replay_outcome(sub)
    assert outcomes_list(out) == want[:n]
    assert (dg == wdg[:n]).all()
    words = (n + 63) // 64
    mask = np.full(words, (1 << 64) - 1, np.uint64)
    if n & 63:
        mask[-1] = np.uint64((1 << (n & 63)) - 1)
    assert (bm == (wbm[:, :words] & mask)).all()
    assert counts.tolist() == [sum(1 for w in want[:n] if w[0] == k) for k in range(dchess.GO_COUNT)]
    assert int(counts.sum()) == n


def test_chunks_share_the_history(engine, seeded):
    """257 games in chunks of 256: two launches, one history buffer, same result."""
    mv, (want, wbm, wcounts, wst, wdg) = seeded[32]
    hook = dchess.lib().dc_test_outcome_chunk_games
    hook.argtypes, hook.restype = [C.c_void_p, C.c_uint32], C.c_int
    engine.set_profiling(True)
    engine.reset_stats()
    assert hook(engine.ctx, 256) == 0
    try:
        out, bm, dg, counts, st = engine.replay_outcome(mv)
        ks = engine.kernel_stats("replay_outcome")
    finally:
        assert hook(engine.ctx, 177664) == 0
        engine.set_profiling(False)
    assert outcomes_list(out) == want and (bm == wbm).all() and (dg == wdg).all()
    assert counts.tolist() == list(wcounts)
    assert {k: st[k] for k in ("validated", "accepted", "rejected")} == wst
    assert ks["launches"] == 2 and ks["units"] == st["validated"]


def test_no_plies(engine):
    mv = np.zeros((0, 65), np.uint16)
    out, bm, dg, counts, st = engine.replay_outcome(mv, start_halfmove=7)
    assert outcomes_list(out) == [(dchess.GO_ONGOING, 0, 1, 7)] * 65
    assert counts.tolist() == [65, 0, 0, 0, 0, 0, 0]
    assert (st["validated"], st["accepted"], st["rejected"]) == (0, 0, 0)
    assert (dg == np.uint64(O.digest(O.startpos_cells(), 0))).all()
    out, _, _, counts, _ = engine.replay_outcome(np.zeros((3, 0), np.uint16))
    assert len(out) == 0 and int(counts.sum()) == 0


@pytest.mark.parametrize("fen,result", [(MATE_FEN, M.BLACK_WINS), (STALE_FEN, M.STALEMATE), (DEAD_FEN, M.DEAD)])
def test_terminal_start(engine, fen, result):
    hm = dchess.fen_clocks(fen)[0]
    pos = O.Pos.from_fen(fen)
    legal_looking = M.line("e1e2 e8e7 a2a3 h8g8")
    mv = np.tile(np.array(legal_looking, np.uint16)[:, None], (1, 3))
    assert M.adjudicate(legal_looking, pos, hm)["result"] == result
    out, bm, dg, counts, st = engine.replay_outcome(mv, dchess.pos_from_fen(fen), hm)
    assert outcomes_list(out) == [(result, 0, 1, hm)] * 3
    assert not bm.any() and st["validated"] == 0 and int(counts[result]) == 3
    assert (dg == np.uint64(O.digest(pos.cells, pos.stm))).all()


def test_clock_above_150_is_einval(engine):
    mv = np.array([[M.mv("e2e4")]], np.uint16)
    with pytest.raises(dchess.DChessError) as e:
        engine.replay_outcome(mv, start_halfmove=151)
    assert e.value.status == dchess.EINVAL
    d_mv, d_out = engine.alloc(2), engine.alloc(8)
    d_mv.upload(mv)
    with pytest.raises(dchess.DChessError) as e:
        engine.replay_outcome_device(d_mv, 1, 1, d_out, start_halfmove=151)
    assert e.value.status == dchess.EINVAL
    counts, _ = engine.replay_outcome_device(d_mv, 1, 1, d_out, start_halfmove=150)
    assert int(counts[dchess.GO_SEVENTYFIVE]) == 1


def test_host_and_device_forms_agree(engine, seeded):
    mv = np.ascontiguousarray(seeded[32][0][:, :65])
    n_plies, n = mv.shape
    words = (n + 63) // 64
    out, bm, dg, counts, st = engine.replay_outcome(mv)
    d_mv, d_out = engine.alloc(mv.nbytes), engine.alloc(8 * n)
    d_bm, d_dg = engine.alloc(8 * words * n_plies), engine.alloc(8 * n)
    d_mv.upload(mv)
    dcounts, dst = engine.replay_outcome_device(d_mv, n, n_plies, d_out, d_bm, d_dg)
    assert (d_out.download(dchess.OUTCOME_DTYPE, n) == out).all()
    assert (d_bm.download(np.uint64, words * n_plies).reshape(n_plies, words) == bm).all()
    assert (d_dg.download(np.uint64, n) == dg).all()
    assert (dcounts == counts).all() and dst == st
    # bitmap and digests are optional
    dcounts, dst = engine.replay_outcome_device(d_mv, n, n_plies, d_out)
    assert (dcounts == counts).all() and dst == st
