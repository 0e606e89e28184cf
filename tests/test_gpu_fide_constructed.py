"""GPU tests of every RULES_FIDE entry point over the constructed positions of
tests/fide_positions.py (640 built from motifs -- en-passant pairs, king lines,
castling, twins -- plus the hand-made ones; tests/test_fide_positions_model.py
asserts what the set holds): legal lists and status, validate over every move
word, apply, perft with divide, perft statistics, and the adjudicating replay
with its SAN bytes.  The expected values are the fastcpu oracle's and the
plain-Python models'; every comparison is exact.

analyse() skips king-line scans for a whole wave, so what a lane computes could
depend on its wave's other lanes: the same positions are therefore also sent in
another order, alone, and interleaved by class."""
import functools

import numpy as np
import pytest

import dchess
import fide_positions as F
import oracle_lib as O
import san_model as S
from test_gpu_legal_moves import Expect, dpos

pytestmark = pytest.mark.gpu

FIDE = dchess.RULES_FIDE
N_SET = F.N_CONSTRUCTED + len(F.HAND)
WORD_CHUNK = 50
REPLAY_CHUNK = 59  # 649 = 11 * 59
PAIRS = np.arange(4096, dtype=np.uint16)


@functools.lru_cache(maxsize=None)
def expect():
    ex = Expect(list(F.position_set()), FIDE)
    assert len(ex.ps) == N_SET == 649
    return ex


@functools.lru_cache(maxsize=None)
def flat():
    """Every legal move of the set: (parent index per move, move words)."""
    ex = expect()
    return np.repeat(np.arange(N_SET), ex.lens), np.concatenate(ex.lists).astype(np.uint16)


def same_pos(a, b):
    """Element-wise equality of two dc_pos arrays in the fields that mean something."""
    a, b = np.atleast_1d(a), np.atleast_1d(b)
    return (a["bb"] == b["bb"]).all(axis=1) & (a["stm"] == b["stm"]) & (a["castle"] == b["castle"]) & (a["ep"] == b["ep"])


def _lists_of(off, mv, st):
    return [(mv[off[i]:off[i + 1]].tolist(), int(st[i])) for i in range(len(st))]


# ------------------------------------------------------ legal lists and status
def test_legal_lists_and_status(engine):
    ex = expect()
    pos, off, mv, st = ex.all()
    goff, gmv, gst = engine.legal_moves(pos, FIDE)
    bad = [i for i, (a, b) in enumerate(zip(_lists_of(goff, gmv, gst), _lists_of(off, mv, st))) if a != b]
    assert not bad, (bad[:5], [dchess.pos_to_fen(pos[i]) for i in bad[:5]])
    # the hand-made positions, by their pinned counts
    assert ex.lens[F.N_CONSTRUCTED:].tolist() == [c for _, c, _ in F.HAND]
    # checkmates, stalemates and both kinds of check are in the expectation
    both = dchess.ST_CHECK | dchess.ST_NO_MOVES
    assert ((st & both) == both).sum() >= 3 and ((st & both) == dchess.ST_NO_MOVES).sum() >= 1
    assert ((st & both) == dchess.ST_CHECK).sum() >= 100


@pytest.mark.parametrize("n", [255, 256, 257])
def test_legal_lists_across_the_one_block_path(engine, n):
    pos, off, mv, st = expect().take(np.arange(n) + 300)
    goff, gmv, gst = engine.legal_moves(pos, FIDE)
    assert (goff == off).all() and (gmv == mv).all() and (gst == st).all()


# --------------------------------------------------- wave-neighbour independence
def test_lists_do_not_depend_on_the_neighbours(engine):
    ex = expect()
    want = _lists_of(*ex.all()[1:])
    perm = np.random.default_rng(11).permutation(N_SET)
    pos, off, mv, st = ex.take(perm)
    got = _lists_of(*engine.legal_moves(pos, FIDE))
    assert [got[j] for j in np.argsort(perm)] == want
    for i in np.random.default_rng(12).choice(N_SET, 32, replace=False).tolist():
        assert _lists_of(*engine.legal_moves(ex.pos[i:i + 1], FIDE)) == [want[i]], i


def test_validate_and_apply_do_not_depend_on_the_neighbours(engine):
    ex = expect()
    par, mv = flat()
    rng = np.random.default_rng(13)
    # every legal move and as many arbitrary words
    par2 = np.concatenate([par, par])
    mv2 = np.concatenate([mv, rng.integers(0, 1 << 15, len(mv)).astype(np.uint16)])
    ver = engine.validate_batch(ex.pos[par2], mv2, FIDE)
    new, aver, info = engine.apply_batch(ex.pos[par2], mv2, FIDE)
    assert (ver[:len(mv)] == dchess.V_OK).all() and (aver == ver).all()
    perm = rng.permutation(len(mv2))
    assert (engine.validate_batch(ex.pos[par2[perm]], mv2[perm], FIDE) == ver[perm]).all()
    pnew, pver, pinfo = engine.apply_batch(ex.pos[par2[perm]], mv2[perm], FIDE)
    assert (pver == ver[perm]).all() and (pinfo == info[perm]).all() and same_pos(pnew, new[perm]).all()


def test_interleaved_and_sorted_waves_agree(engine):
    """Lane by lane, a position with an enemy slider on a line of its king beside
    one with none (every wave's gates are split), then the same positions with
    whole waves of one class."""
    ex = expect()
    has = np.array([F.slider_on_king_line(p) for p in ex.ps])
    a, b = np.flatnonzero(has), np.flatnonzero(~has)
    k = min(len(a), len(b))
    assert k >= 128  # two whole waves of each class
    mixed = np.stack([a[:k], b[:k]], axis=1).reshape(-1)
    sorted_ = np.concatenate([a[:k], b[:k]])
    assert not has[mixed[1::2]].any() and has[mixed[0::2]].all() and has[sorted_[:k]].all()
    want = _lists_of(*ex.all()[1:])
    for idx in (mixed, sorted_):
        pos, off, mv, st = ex.take(idx)
        assert _lists_of(*engine.legal_moves(pos, FIDE)) == [want[i] for i in idx.tolist()]
        # the per-move paths over the same lanes: each position's first legal move and one fixed word
        first = np.array([ex.lists[i][0] if ex.lens[i] else 0 for i in idx.tolist()], np.uint16)
        okay = np.array([dchess.V_OK if ex.lens[i] else O.fast_validate(ex.ps[i], 0, O.FIDE) for i in idx.tolist()])
        assert (engine.validate_batch(pos, first, FIDE) == okay).all()
        new, ver, _ = engine.apply_batch(pos, first, FIDE)
        assert (ver == okay).all()
        for j in range(0, len(idx), 7):
            if okay[j] == dchess.V_OK:
                q = dpos(O.fast_make(ex.ps[idx[j]], int(first[j]), O.FIDE))
                assert same_pos(new[j:j + 1], np.array([q], dchess.POS_DTYPE)).all(), j


# ------------------------------------------------------------- every move word
@pytest.mark.parametrize("chunk", range((N_SET + WORD_CHUNK - 1) // WORD_CHUNK))
def test_every_move_word(engine, chunk):
    """All 4,096 (from, to) pairs with promotion codes 0..4 of WORD_CHUNK positions a call."""
    ex = expect()
    idx = np.arange(chunk * WORD_CHUNK, min(N_SET, (chunk + 1) * WORD_CHUNK))
    words = np.concatenate([PAIRS | np.uint16(pr << 12) for pr in range(5)])
    want = np.stack([F.verdict_table(ex.ps[i], ex.lists[i]).reshape(-1) for i in idx.tolist()])
    assert ((want == O.OK).sum(axis=1) == ex.lens[idx]).all()
    # the vectorised table itself, against the oracle's validate (2,000 words over the chunks)
    rng = np.random.default_rng(100 + chunk)
    for r, c in zip(rng.integers(0, len(idx), 154).tolist(), rng.integers(0, len(words), 154).tolist()):
        assert want[r, c] == O.fast_validate(ex.ps[idx[r]], int(words[c]), O.FIDE)
    got = engine.validate_batch(np.repeat(ex.pos[idx], len(words)), np.tile(words, len(idx)), FIDE)
    got = got.reshape(len(idx), len(words))
    bad = np.argwhere(got != want)
    assert len(bad) == 0, [(int(idx[r]), dchess.pos_to_fen(ex.pos[idx[r]]), hex(int(words[c])), int(got[r, c]),
                            int(want[r, c])) for r, c in bad[:5]]


def test_promotion_codes_5_to_7_and_flagged_words(engine):
    ex = expect()
    idx = np.random.default_rng(14).choice(N_SET, 32, replace=False)
    assert sum(any(int(m) >> 12 for m in ex.lists[i]) for i in idx.tolist()) >= 1  # a position that can promote
    high = np.concatenate([PAIRS | np.uint16(pr << 12) for pr in (5, 6, 7)])
    flagged = np.concatenate([PAIRS | np.uint16(0x8000), PAIRS | np.uint16(0xC000), PAIRS | np.uint16(0xF000)])
    words = np.concatenate([high, flagged])
    want = np.empty((32, len(words)), np.uint8)
    for r, i in enumerate(idx.tolist()):
        want[r, :len(high)] = F.verdict_table(ex.ps[i], ex.lists[i], (5, 6, 7)).reshape(-1)
        want[r, len(high):] = O.OOR
    assert not (want == O.OK).any() and words[-1] == 0xFFFF
    rng = np.random.default_rng(15)
    for r, c in zip(rng.integers(0, 32, 300).tolist(), rng.integers(0, len(words), 300).tolist()):
        assert want[r, c] == O.fast_validate(ex.ps[idx[r]], int(words[c]), O.FIDE)
    got = engine.validate_batch(np.repeat(ex.pos[idx], len(words)), np.tile(words, 32), FIDE).reshape(32, -1)
    assert (got == want).all()
    # apply leaves a rejected position untouched
    pos = np.repeat(ex.pos[idx], 64)
    sub = np.tile(words[::len(words) // 64][:64], 32)
    new, ver, info = engine.apply_batch(pos, sub, FIDE)
    assert (ver != dchess.V_OK).all() and same_pos(new, pos).all() and (info == 0xFF).all()


# ----------------------------------------------------------------------- apply
def test_apply_every_legal_move(engine):
    ex = expect()
    par, mv = flat()
    kids = [O.fast_make(ex.ps[i], int(m), O.FIDE) for i, m in zip(par.tolist(), mv.tolist())]
    want = np.array([dpos(q) for q in kids], dchess.POS_DTYPE)
    cells = np.stack([p.cells for p in ex.ps]).astype(np.int64)
    f, t, promo = (mv & 63).astype(np.int64), ((mv >> 6) & 63).astype(np.int64), (mv >> 12).astype(np.int64)
    kind = cells[par, f] & 7
    winfo = (kind | np.where(cells[par, t] >= 0, 8, 0)).astype(np.uint8)
    # what the sample holds, on the CPU side
    castles = (kind == F.K) & (np.abs(t - f) == 2)
    assert castles.sum() >= 100
    for j in np.flatnonzero(castles)[:50].tolist():   # the rook has moved beside the king
        assert kids[j].cells[(f[j] + t[j]) // 2] == ex.ps[par[j]].stm * 8 + F.R
    corner_right = {0: 2, 7: 1, 56: 8, 63: 4}
    lost = [j for j in range(len(mv)) if int(t[j]) in corner_right and cells[par[j], t[j]] >= 0
            and (cells[par[j], t[j]] & 7) == F.R and ex.ps[par[j]].castle & corner_right[int(t[j])]
            and not kids[j].castle & corner_right[int(t[j])]]
    assert len(lost) >= 5                              # a rook captured on its corner takes the right with it
    eps = np.flatnonzero((kind == F.P) & (t == np.array([ex.ps[i].ep for i in par.tolist()])) & ((f & 7) != (t & 7)))
    assert len(eps) >= 150
    for j in eps[:50].tolist():                        # the pawn beside the capturer is gone
        assert kids[j].cells[(f[j] & ~7) | (t[j] & 7)] == -1 and winfo[j] == F.P
    assert all((promo == k).sum() >= 50 for k in (1, 2, 3, 4))
    new, ver, info = engine.apply_batch(ex.pos[par], mv, FIDE)
    assert (ver == dchess.V_OK).all()
    for field in ("bb", "stm", "castle", "ep"):
        bad = np.flatnonzero((new[field] != want[field]).reshape(len(mv), -1).any(axis=1))
        assert len(bad) == 0, (field, [(dchess.pos_to_fen(ex.pos[par[j]]), hex(int(mv[j]))) for j in bad[:5]])
    assert (info == winfo).all()


# ----------------------------------------------------------------------- perft
@pytest.mark.parametrize("depth", [1, 2, 3])
def test_perft_with_divide(engine, depth):
    """The whole set at every depth: depth 3 is 10.2 M leaves in all and runs in
    well under a second, so no subset is taken."""
    ex = expect()
    leaves = 0
    for i, p in enumerate(ex.ps):
        tot, div, rm = engine.perft(ex.pos[i], depth, FIDE)
        otot, odiv, orm = O.fast_perft(p, depth, O.FIDE, threads=1 if depth < 3 else None)
        assert tot == otot, (i, dchess.pos_to_fen(ex.pos[i]), tot, otot)
        assert dict(zip(rm.tolist(), div.tolist())) == dict(zip(orm.tolist(), odiv.tolist())), i
        assert len(rm) == ex.lens[i]
        leaves += tot
    assert leaves > 0 and (depth > 1 or leaves == int(ex.lens.sum()))


# ------------------------------------------------------------ perft statistics
def test_perft_stats_depth1_rows(engine):
    ex = expect()
    seen = np.zeros(F.PS_COUNT, np.int64)
    for i, p in enumerate(ex.ps):
        wtot, wrows = F.stats_below(p, 1)
        tot, rows, rm = engine.perft_stats(ex.pos[i], 1, FIDE)
        assert tot.tolist() == wtot, (i, dchess.pos_to_fen(ex.pos[i]), tot.tolist(), wtot)
        got = {int(m): [int(v) for v in r] for m, r in zip(rm, rows)}
        assert got == wrows, (i, dchess.pos_to_fen(ex.pos[i]))
        seen += tot.astype(np.int64)
    assert seen[F.PS_DISCOVERED] >= 100 and seen[F.PS_DOUBLE] >= 5 and seen[F.PS_STALEMATES] >= 5


@pytest.mark.parametrize("half", [0, 1])
def test_perft_stats_depth2_totals(engine, half):
    """A seeded subset of 150 positions (rng 16, without replacement), 75 a case:
    the model applied below the oracle's first ply."""
    ex = expect()
    idx = np.random.default_rng(16).choice(N_SET, 150, replace=False)[75 * half:75 * half + 75]
    for i in idx.tolist():
        wtot, wrows = F.stats_below(ex.ps[i], 2)
        tot, rows, rm = engine.perft_stats(ex.pos[i], 2, FIDE)
        assert tot.tolist() == wtot, (i, dchess.pos_to_fen(ex.pos[i]), tot.tolist(), wtot)
        assert {int(m): [int(v) for v in r] for m, r in zip(rm, rows)} == wrows, i


# ------------------------------------------------- adjudicated replay with SAN
def replay_games(i):
    """Position i's games: one per legal move, then a seeded legal reply, then a
    word that is never legal (from == to).  Where the reply can be an en-passant
    capture of the pawn that just pushed, or a castle, it is one half of the
    time: those read back the ep square and the rights the first ply's make
    left.  A position without a legal move gets one game, which must end
    before its first ply."""
    ex = expect()
    p, legal = ex.ps[i], ex.lists[i]
    rng = np.random.default_rng(1000 + i)
    n = max(1, len(legal))
    mv = np.full((3, n), 0xFFFF, np.uint16)
    for g, m in enumerate(legal.tolist()):
        mv[0, g] = m
        child = O.fast_make(p, m, O.FIDE)
        reply = O.fast_gen_moves(child, O.FIDE)
        if len(reply):
            rf, rt = reply & 63, (reply >> 6) & 63
            kind = child.cells[rf] & 7
            special = reply[((kind == F.P) & (rt == child.ep) & ((rf & 7) != (rt & 7)))
                            | ((kind == F.K) & (np.abs(rf.astype(int) - rt.astype(int)) == 2))]
            pick = special if len(special) and rng.random() < 0.5 else reply
            mv[1, g] = pick[int(rng.integers(0, len(pick)))]
    if not len(legal):
        mv[0, 0] = int(rng.integers(0, 4096))
    s = rng.integers(0, 64, n).astype(np.uint16)
    mv[2] = s | (s << 6)
    return mv


def replay_expectation(i, mv, hm):
    p = expect().ps[i]
    rs = [S.annotate(mv[:, g], p, hm) for g in range(mv.shape[1])]
    n = len(rs)
    out = np.zeros(n, dchess.OUTCOME_DTYPE)
    bitmap = np.zeros((3, (n + 63) // 64), np.uint64)
    for g, r in enumerate(rs):
        out[g] = (r["result"], r["repeats"], r["halfmove"], r["end_ply"])
        for ply, ok in enumerate(r["accept"]):
            if ok:
                bitmap[ply, g >> 6] |= np.uint64(1 << (g & 63))
    san = np.array([r["san"] for r in rs], np.uint8).T.reshape(3, n)
    dig = np.array([O.digest(r["pos"].cells, r["pos"].stm) for r in rs], np.uint64)
    counts = np.bincount(out["result"], minlength=dchess.GO_COUNT).astype(np.uint64)
    val, acc = sum(r["validated"] for r in rs), sum(r["accepted"] for r in rs)
    return out, san, bitmap, dig, counts, {"validated": val, "accepted": acc, "rejected": val - acc}


@pytest.mark.parametrize("chunk", range((N_SET + REPLAY_CHUNK - 1) // REPLAY_CHUNK))
def test_replay_san(engine, chunk):
    ex = expect()
    second_ply_special = 0
    for i in range(chunk * REPLAY_CHUNK, min(N_SET, (chunk + 1) * REPLAY_CHUNK)):
        hm = 99 if i & 1 else 0
        mv = replay_games(i)
        wout, wsan, wbm, wdg, wcounts, wst = replay_expectation(i, mv, hm)
        out, san, bm, dg, counts, st = engine.replay_san(mv, start=ex.pos[i], start_halfmove=hm)
        where = (i, dchess.pos_to_fen(ex.pos[i], hm))
        assert (san == wsan).all(), (where, np.argwhere(san != wsan)[:5].tolist())
        assert (out == wout).all(), where
        assert (bm == wbm).all() and (dg == wdg).all(), where
        assert (counts == wcounts).all(), where
        assert {k: st[k] for k in wst} == wst, where
        # the third ply is never accepted, and the first always unless the start is terminal (no move, dead)
        assert (san[2] == S.NONE).all() and ((san[0] != S.NONE) == (wout["end_ply"] > 0)).all()
        # second plies that read back the state the first one left: an en-passant reply, a castle
        f, t = mv[1] & 63, (mv[1] >> 6) & 63
        second_ply_special += int(((san[1] != S.NONE) & ((san[1] & 7) == F.P) & ((san[1] & S.CAPTURE) != 0)
                                   & (np.abs((mv[0] & 63).astype(int) - ((mv[0] >> 6) & 63)) == 16)
                                   & (t == ((mv[0] & 63) + ((mv[0] >> 6) & 63)) // 2)).sum())
        second_ply_special += int(((san[1] != S.NONE) & ((san[1] & 7) == F.K)
                                   & (np.abs(f.astype(int) - t.astype(int)) == 2)).sum())
    assert second_ply_special >= 1


def test_three_queens_need_file_and_rank(engine):
    """Qh1e4 with queens on h4 and e1 as well: the byte carries FILE | RANK, and the formatter writes both."""
    fen = "8/k7/8/8/7Q/8/8/K3Q2Q w - - 0 1"
    assert fen in [f for f, _, _ in F.HAND]
    mv = np.array([[S.M.mv("h1e4"), S.M.mv("h4e4"), S.M.mv("e1e4"), S.M.mv("h1h3")]], np.uint16)
    san = engine.replay_san(mv, start=dchess.pos_from_fen(fen))[1]
    assert (san[0] & (S.FILE | S.RANK)).tolist() == [S.FILE | S.RANK, S.RANK, S.FILE, S.RANK]
    assert [dchess.san_format(int(m), int(b)) for m, b in zip(mv[0], san[0])] == ["Qh1e4", "Q4e4", "Qee4", "Q1h3"]


# ---------------------------------------------------------------- device forms
def test_legal_moves_device_form(engine):
    pos, off, mv, st = expect().take(np.arange(300))
    n, total = len(pos), len(mv)
    d_pos, d_off, d_st, d_mv = engine.alloc(pos.nbytes), engine.alloc(4 * (n + 1)), engine.alloc(n), engine.alloc(2 * total)
    try:
        d_pos.upload(pos)
        assert engine.legal_moves_device(d_pos, n, d_off, d_st, d_mv, total, FIDE) == total
        assert (d_off.download(np.uint32, n + 1) == off).all()
        assert (d_mv.download(np.uint16, total) == mv).all()
        assert (d_st.download(np.uint8, n) == st).all()
    finally:
        for d in (d_pos, d_off, d_st, d_mv):
            d.free()


def test_replay_san_device_form(engine):
    ex = expect()
    i = int(np.argmax(ex.lens))  # the position with the most games: more than one wave
    assert ex.lens[i] > 64
    mv = replay_games(i)
    wout, wsan, wbm, wdg, wcounts, wst = replay_expectation(i, mv, 99)
    n_plies, n = mv.shape
    words = (n + 63) // 64
    bufs = [engine.alloc(mv.nbytes), engine.alloc(8 * n), engine.alloc(n * n_plies), engine.alloc(8 * words * n_plies),
            engine.alloc(8 * n)]
    d_mv, d_out, d_san, d_bm, d_dg = bufs
    try:
        d_mv.upload(mv)
        counts, st = engine.replay_san_device(d_mv, n, n_plies, d_out, d_san, d_bm, d_dg, start=ex.pos[i],
                                              start_halfmove=99)
        assert (d_out.download(dchess.OUTCOME_DTYPE, n) == wout).all()
        assert (d_san.download(np.uint8, n * n_plies).reshape(n_plies, n) == wsan).all()
        assert (d_bm.download(np.uint64, words * n_plies).reshape(n_plies, words) == wbm).all()
        assert (d_dg.download(np.uint64, n) == wdg).all()
        assert (counts == wcounts).all() and {k: st[k] for k in wst} == wst
    finally:
        for d in bufs:
            d.free()
