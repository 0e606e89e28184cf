"""GPU tests of dc_legal_moves_batch / dc_legal_moves_batch_device: the legal
moves of a batch of positions as a dense CSR in canonical (from, to, promo)
order, and the status byte (check, no moves, dead position).

The move lists are pinned by the independent fastcpu mailbox engine
(oracle_lib.fast_gen_moves, canonical order, at most 256 moves per position --
every test position stays within that); CHECK and DEAD by a mailbox attack
test and a material count written here, independent of the kernels' bitboard
code.  Every FIDE test position has exactly one king per side."""
import functools
import json
import os

import numpy as np
import pytest

import dchess
import oracle_lib as O

pytestmark = pytest.mark.gpu

OG = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "oracle_golden.json")))
REF, FIDE = dchess.RULES_REF, dchess.RULES_FIDE

# FEN, FIDE move count, in check
HAND = [
    ("rnb1kbnr/pppp1ppp/8/4p3/6Pq/5P2/PPPPP2P/RNBQKBNR w KQkq - 1 3", 0, True),   # mate
    ("7k/5Q2/6K1/8/8/8/8/8 b - - 0 1", 0, False),                                  # stalemate
    ("4k3/8/5N2/8/8/8/8/4RK2 b - - 0 1", 3, True),                                 # double check
    ("8/8/8/8/k2Pp2Q/8/8/3K4 b - d3 0 1", 6, False),                               # ep pinned on the rank: excluded
    ("8/8/8/8/3Pp3/8/8/k2K4 b - d3 0 1", 5, False),                                # ep included
    ("n1n5/PPPk4/8/8/8/8/4Kppp/5N1N b - - 0 1", 24, False),
    ("r3k2r/8/8/8/4Q3/8/8/4K3 b kq - 0 1", 4, True),
    ("R6R/3Q4/1Q4Q1/4Q3/2Q4Q/Q4Q2/pp1Q4/kBNN1KB1 w - - 0 1", 218, False),
]
FEN_218 = HAND[7][0]
DEAD_FENS = ["8/8/8/4k3/8/8/8/4K3 w - - 0 1", "8/8/8/4k3/8/8/8/4KB2 w - - 0 1", "8/8/8/4k3/8/8/8/4KN2 b - - 0 1",
             "8/8/8/4kb2/8/8/8/4KB2 w - - 0 1"]
LIVE_FENS = ["8/8/8/4k1b1/8/8/8/4KB2 w - - 0 1", "8/8/8/4k3/8/8/8/3NKN2 w - - 0 1", "8/8/8/4k3/8/4P3/8/4K3 w - - 0 1"]
# candidates for a position with exactly one legal move (the oracle confirms one)
ONE_MOVE_FENS = ["kr6/8/8/8/8/8/8/K6r w - - 0 1", "7k/8/8/8/8/8/r7/1r5K w - - 0 1"]

P, N, B, R, Q, K, X = range(7)  # cell kinds


def dpos(p):
    d = dchess.pos_from_cells(p.cells, p.stm)
    d["castle"], d["ep"] = p.castle, p.ep
    return d


def _random_positions(n, seed, rules):
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


# ------------------------------------------------ mailbox status (independent)
def _attacked(cells, x, y, by):
    """Is square (x, y) attacked by a piece of colour `by` (mailbox scan)?"""
    def at(i, j):
        return int(cells[8 * i + j]) if 0 <= i < 8 and 0 <= j < 8 else None

    def is_(i, j, kinds):
        c = at(i, j)
        return c is not None and c >= 0 and (c >> 3) == by and (c & 7) in kinds

    px = x + 1 if by == 1 else x - 1  # a black pawn attacks toward lower x, a white one toward higher x
    if is_(px, y - 1, (P,)) or is_(px, y + 1, (P,)):
        return True
    for dx, dy in ((1, 2), (2, 1), (-1, 2), (-2, 1), (1, -2), (2, -1), (-1, -2), (-2, -1)):
        if is_(x + dx, y + dy, (N,)):
            return True
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            if (dx or dy) and is_(x + dx, y + dy, (K,)):
                return True
    for dirs, kinds in ((((1, 0), (-1, 0), (0, 1), (0, -1)), (R, Q)), (((1, 1), (1, -1), (-1, 1), (-1, -1)), (B, Q))):
        for dx, dy in dirs:
            i, j = x + dx, y + dy
            while at(i, j) is not None:
                if at(i, j) >= 0:
                    if is_(i, j, kinds):
                        return True
                    break
                i, j = i + dx, j + dy
    return False


def in_check(p):
    ks = [s for s in range(64) if p.cells[s] == p.stm * 8 + K]
    assert len(ks) == 1
    return _attacked(p.cells, ks[0] >> 3, ks[0] & 7, 1 - p.stm)


def is_dead(p):
    kinds = [int(c) & 7 for c in p.cells if c >= 0]
    if any(k in (P, R, Q, X) for k in kinds):
        return False
    minors = [s for s in range(64) if p.cells[s] >= 0 and (int(p.cells[s]) & 7) in (N, B)]
    if len(minors) <= 1:
        return True
    if any((int(p.cells[s]) & 7) == N for s in minors):
        return False
    return len({((s >> 3) + (s & 7)) & 1 for s in minors}) == 1


class Expect:
    """Oracle lists and expected status of a position set under one rule set."""

    def __init__(self, ps, rules):
        self.ps = ps
        self.rules = rules
        self.pos = np.array([dpos(p) for p in ps], dchess.POS_DTYPE)
        self.lists = [O.fast_gen_moves(p, rules) for p in ps]
        self.lens = np.array([len(m) for m in self.lists], np.int64)
        assert self.lens.max(initial=0) < 256  # the oracle's buffer holds 256
        st = []
        for p, m in zip(ps, self.lists):
            s = dchess.ST_NO_MOVES if len(m) == 0 else 0
            if rules == FIDE:
                s |= (dchess.ST_CHECK if in_check(p) else 0) | (dchess.ST_DEAD if is_dead(p) else 0)
            st.append(s)
        self.status = np.array(st, np.uint8)

    def take(self, idx):
        """(positions, offsets, moves, status) of the positions idx (an index array)."""
        idx = np.asarray(idx)
        off = np.zeros(len(idx) + 1, np.uint32)
        off[1:] = np.cumsum(self.lens[idx])
        parts = [self.lists[i] for i in idx.tolist()]
        mv = np.concatenate(parts) if parts else np.zeros(0, np.uint16)
        return self.pos[idx], off, mv.astype(np.uint16), self.status[idx]

    def all(self):
        return self.take(np.arange(len(self.ps)))


def _check(engine, ex_take, rules):
    pos, off, mv, st = ex_take
    goff, gmv, gst = engine.legal_moves(pos, rules)
    assert (goff == off).all()
    assert len(gmv) == len(mv) and (gmv == mv).all()
    assert (gst == st).all()


@functools.lru_cache(maxsize=None)
def fide_random():
    return _random_positions(600, 71, O.FIDE)


@functools.lru_cache(maxsize=None)
def fide_set():
    """The 615-position FIDE set: random, the six suite positions, the hand-made ones."""
    ps = list(fide_random())
    ps += [O.Pos.from_fen(e["fen"]) for e in OG["perft_fide"].values()]
    ps += [O.Pos.from_fen(f) for f, _, _ in HAND]
    ps += [O.Pos.from_fen(ONE_MOVE_FENS[0])]
    assert len(ps) == 615
    return Expect(ps, FIDE)


@functools.lru_cache(maxsize=None)
def one_move_pos():
    for f in ONE_MOVE_FENS:
        p = O.Pos.from_fen(f)
        if len(O.fast_gen_moves(p, O.FIDE)) == 1:
            return p
    for p in fide_random():
        if len(O.fast_gen_moves(p, O.FIDE)) == 1:
            return p
    raise AssertionError("no one-move position")


@functools.lru_cache(maxsize=None)
def ref_random():
    return Expect(_random_positions(600, 72, O.REF), REF)


@functools.lru_cache(maxsize=None)
def ref_junk():
    rng = np.random.default_rng(5)
    ps = []
    for _ in range(400):
        cells = np.full(64, -1, np.int8)
        k = int(rng.integers(0, 40))
        sq = rng.choice(64, k, replace=False)
        cells[sq] = rng.integers(0, 2, k) * 8 + rng.integers(0, 7, k)
        ps.append(O.Pos(cells, int(rng.integers(0, 2))))
    ps.append(O.Pos(np.full(64, -1, np.int8), 0))  # the empty board
    return Expect(ps, REF)


# -------------------------------------------------------------------- parity
def test_fide_random_set_coverage_and_parity(engine):
    ps = fide_random()
    lists = [O.fast_gen_moves(p, O.FIDE) for p in ps]
    assert sum(in_check(p) for p in ps) >= 20
    assert sum(len(m) == 0 for m in lists) >= 5
    assert sum(p.ep >= 0 for p in ps) >= 20
    assert sum(p.castle != 0 for p in ps) >= 100
    assert sum(any(int(x) >> 12 for x in m) for m in lists) >= 5
    ex = Expect(ps, FIDE)
    _check(engine, ex.all(), FIDE)


def test_fide_suite_positions(engine):
    ex = Expect([O.Pos.from_fen(e["fen"]) for e in OG["perft_fide"].values()], FIDE)
    assert len(ex.ps) == 6
    _check(engine, ex.all(), FIDE)


def test_fide_hand_made_positions(engine):
    ex = Expect([O.Pos.from_fen(f) for f, _, _ in HAND], FIDE)
    # the table itself, against the oracle and the mailbox attack test
    assert ex.lens.tolist() == [c for _, c, _ in HAND]
    assert [in_check(p) for p in ex.ps] == [k for _, _, k in HAND]
    _check(engine, ex.all(), FIDE)
    _, _, st = engine.legal_moves(ex.pos, FIDE)
    assert st[0] == dchess.ST_CHECK | dchess.ST_NO_MOVES  # checkmate
    assert st[1] == dchess.ST_NO_MOVES                    # stalemate
    assert st[2] == dchess.ST_CHECK


def test_fide_dead_positions(engine):
    dead = Expect([O.Pos.from_fen(f) for f in DEAD_FENS], FIDE)
    live = Expect([O.Pos.from_fen(f) for f in LIVE_FENS], FIDE)
    assert all(s & dchess.ST_DEAD for s in dead.status) and not any(s & dchess.ST_DEAD for s in live.status)
    _check(engine, dead.all(), FIDE)
    _check(engine, live.all(), FIDE)


def test_ref_random_set(engine):
    ex = ref_random()
    assert ex.lens.min() >= 1
    assert not ex.status.any()
    _check(engine, ex.all(), REF)


def test_ref_junk_boards(engine):
    ex = ref_junk()
    assert (ex.lens == 0).sum() >= 10 and ex.lens.max() >= 60
    assert ex.lens[-1] == 0  # the empty board
    _check(engine, ex.all(), REF)


def test_fide_positions_under_ref_ignore_castle_and_ep(engine):
    ex = Expect(fide_random(), REF)
    assert (ex.pos["castle"] != 0).any() and (ex.pos["ep"] >= 0).any()
    _check(engine, ex.all(), REF)
    # REF never sets CHECK or DEAD
    dead = Expect([O.Pos.from_fen(f) for f in DEAD_FENS] + [O.Pos.from_fen(HAND[0][0])], REF)
    assert not (dead.status & (dchess.ST_CHECK | dchess.ST_DEAD)).any()
    _check(engine, dead.all(), REF)


# --------------------------------------------------------------- batch shapes
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 615, 70001])
def test_batch_shapes(engine, n):
    ex = fide_set()
    idx = np.arange(n) % 615
    if n in (256, 257):
        engine.set_profiling(True)
        engine.reset_stats()
    try:
        _check(engine, ex.take(idx), FIDE)
        if n in (256, 257):
            emit, small = engine.kernel_stats("legal_emit"), engine.kernel_stats("legal_small")
            count = engine.kernel_stats("legal_count")
            if n == 256:  # one block: the fused kernel, sizing and fill
                assert small["launches"] == 2 and emit["launches"] == 0 and count["launches"] == 0
            else:         # the three-launch path
                assert emit["launches"] == 1 and count["launches"] == 2 and small["launches"] == 0
                assert count["units"] == 2 * n and emit["units"] == int(ex.lens[idx].sum())
    finally:
        if n in (256, 257):
            engine.set_profiling(False)
            engine.reset_stats()


# -------------------------------------------------------------- staging edges
def test_staging_every_wave_overflows_one_chunk(engine):
    ex = Expect([O.Pos.from_fen(FEN_218)], FIDE)
    assert ex.lens[0] == 218
    for n in (128, 300):  # one block (fused) and two blocks (three launches)
        _check(engine, ex.take(np.zeros(n, np.int64)), FIDE)


def test_staging_waves_without_output(engine):
    ex = Expect([O.Pos.from_fen(HAND[0][0]), O.Pos.from_fen(HAND[1][0])], FIDE)
    assert (ex.lens == 0).all()
    for n in (192, 320):
        pos, off, mv, st = ex.take(np.arange(n) % 2)
        assert len(mv) == 0
        _check(engine, (pos, off, mv, st), FIDE)


def test_staging_alternating_218_0_1(engine):
    ex = Expect([O.Pos.from_fen(FEN_218), O.Pos.from_fen(HAND[0][0]), one_move_pos()], FIDE)
    assert ex.lens.tolist() == [218, 0, 1]
    for n in (192, 515):
        _check(engine, ex.take(np.arange(n) % 3), FIDE)
    # odd starts of every wave's run: a one-move position first
    _check(engine, ex.take((np.arange(515) + 2) % 3), FIDE)


# ----------------------------------------------------------- capacity contract
def _host_call(engine, pos, rules, moves, cap):
    n = len(pos)
    off = np.full(n + 1, 0xDEADBEEF, np.uint32)
    st = np.full(n, 0xEE, np.uint8)
    import ctypes as C
    tot = C.c_uint32(0xDEADBEEF)
    rc = dchess.lib().dc_legal_moves_batch(engine.ctx, rules, dchess._ptr(pos), n, dchess._ptr(off), dchess._ptr(st),
                                           dchess._ptr(moves), cap, C.byref(tot))
    return rc, off, st, tot.value


@pytest.mark.parametrize("n", [200, 615])
def test_capacity_contract_host(engine, n):
    pos, off, mv, st = fide_set().take(np.arange(n))
    total = len(mv)
    # sizing call
    rc, goff, gst, gtot = _host_call(engine, pos, FIDE, None, 0)
    assert rc == dchess.SUCCESS and gtot == total and (goff == off).all() and (gst == st).all()
    # a non-NULL buffer with moves_cap == 0 also only sizes
    buf = np.full(total + 64, 0xFFFF, np.uint16)
    rc, goff, gst, gtot = _host_call(engine, pos, FIDE, buf, 0)
    assert rc == dchess.SUCCESS and gtot == total and (goff == off).all() and (buf == 0xFFFF).all()
    # exact capacity: the guard words stay
    rc, goff, gst, gtot = _host_call(engine, pos, FIDE, buf, total)
    assert rc == dchess.SUCCESS and gtot == total and (goff == off).all() and (gst == st).all()
    assert (buf[:total] == mv).all() and (buf[total:] == 0xFFFF).all()
    # one short: DC_EINVAL, nothing written into moves, the rest still correct
    buf[:] = 0xFFFF
    rc, goff, gst, gtot = _host_call(engine, pos, FIDE, buf, total - 1)
    assert rc == dchess.EINVAL and (buf == 0xFFFF).all()
    assert gtot == total and (goff == off).all() and (gst == st).all()


@pytest.mark.parametrize("n", [200, 615])
def test_capacity_contract_device(engine, n):
    pos, off, mv, st = fide_set().take(np.arange(n))
    total = len(mv)
    d_pos = engine.alloc(pos.nbytes)
    d_pos.upload(pos)
    d_off, d_st = engine.alloc(4 * (n + 1)), engine.alloc(n)
    d_mv = engine.alloc(2 * (total + 64))
    fill = np.full(total + 64, 0xFFFF, np.uint16)
    try:
        d_mv.upload(fill)
        assert engine.legal_moves_device(d_pos, n, d_off, d_st, None, 0, FIDE) == total
        assert (d_off.download(np.uint32, n + 1) == off).all()
        assert engine.legal_moves_device(d_pos, n, d_off, d_st, d_mv, total, FIDE) == total
        got = d_mv.download(np.uint16, total + 64)
        assert (got[:total] == mv).all() and (got[total:] == 0xFFFF).all()
        assert (d_off.download(np.uint32, n + 1) == off).all() and (d_st.download(np.uint8, n) == st).all()
        d_mv.upload(fill)
        d_off.upload(np.zeros(n + 1, np.uint32))
        with pytest.raises(dchess.DChessError) as e:
            engine.legal_moves_device(d_pos, n, d_off, d_st, d_mv, total - 1, FIDE)
        assert e.value.status == dchess.EINVAL
        assert (d_mv.download(np.uint16, total + 64) == 0xFFFF).all()
        assert (d_off.download(np.uint32, n + 1) == off).all()
    finally:
        for d in (d_pos, d_off, d_st, d_mv):
            d.free()


def test_argument_errors(engine):
    pos, off, mv, st = fide_set().take(np.arange(3))
    import ctypes as C
    L = dchess.lib()
    o = np.full(4, 7, np.uint32)
    assert L.dc_legal_moves_batch(engine.ctx, 2, dchess._ptr(pos), 3, dchess._ptr(o), None, None, 0, None) == dchess.EINVAL
    assert L.dc_legal_moves_batch(engine.ctx, FIDE, None, 3, dchess._ptr(o), None, None, 0, None) == dchess.EINVAL
    assert L.dc_legal_moves_batch(engine.ctx, FIDE, dchess._ptr(pos), 3, None, None, None, 0, None) == dchess.EINVAL
    assert L.dc_legal_moves_batch(engine.ctx, FIDE, None, 0, dchess._ptr(o), None, None, 0, None) == dchess.SUCCESS
    assert o[0] == 0
    # status and total are optional
    assert L.dc_legal_moves_batch(engine.ctx, FIDE, dchess._ptr(pos), 3, dchess._ptr(o), None, None, 0, None) == dchess.SUCCESS
    assert (o == off).all()
    # stm is taken as stm & 1
    q = pos.copy()
    q["stm"] |= 2
    goff, gmv, gst = engine.legal_moves(q, FIDE)
    assert (goff == off).all() and (gmv == mv).all() and (gst == st).all()


# ------------------------------------------------- agreement with the old API
@pytest.mark.parametrize("rules", [FIDE, REF])
def test_agrees_with_perft_and_validate(engine, rules):
    ex = fide_set() if rules == FIDE else ref_random()
    pos, off, mv, st = ex.take(np.arange(64))
    goff, gmv, _ = engine.legal_moves(pos, rules)
    assert (goff == off).all() and (gmv == mv).all()
    # dc_perft lists its root moves in its generator's order (move class by
    # move class), not in (from, to, promo) order: the same moves, each once,
    # which put in canonical order are the list
    canon = lambda m: (m & 63, (m >> 6) & 63, m >> 12)  # noqa: E731
    for i in range(64):
        mine = gmv[goff[i]:goff[i + 1]].tolist()
        _, _, rm = engine.perft(pos[i], 1, rules)
        assert len(set(rm.tolist())) == len(rm) == len(mine), i
        assert sorted(rm.tolist(), key=canon) == mine, i
    # every listed move is accepted
    rep = np.repeat(pos, np.diff(goff.astype(np.int64)))
    assert (engine.validate_batch(rep, gmv, rules) == dchess.V_OK).all()
    # and nothing else: all 4,096 pairs (FIDE: with every promotion code) per position
    pairs = np.arange(4096, dtype=np.uint16)
    words = np.concatenate([pairs | np.uint16(pr << 12) for pr in (range(5) if rules == FIDE else range(1))])
    ver = engine.validate_batch(np.repeat(pos, len(words)), np.tile(words, 64), rules).reshape(64, len(words))
    assert ((ver == dchess.V_OK).sum(axis=1) == np.diff(goff.astype(np.int64))).all()


def test_device_form_equals_host_form(engine):
    pos, off, mv, st = fide_set().all()
    n = len(pos)
    hoff, hmv, hst = engine.legal_moves(pos, FIDE)
    d_pos = engine.alloc(pos.nbytes)
    d_pos.upload(pos)
    d_off, d_st, d_mv = engine.alloc(4 * (n + 1)), engine.alloc(n), engine.alloc(2 * len(hmv))
    try:
        tot = engine.legal_moves_device(d_pos, n, d_off, d_st, d_mv, len(hmv), FIDE)
        assert tot == len(hmv) == int(hoff[-1])
        assert (d_off.download(np.uint32, n + 1) == hoff).all()
        assert (d_mv.download(np.uint16, tot) == hmv).all()
        assert (d_st.download(np.uint8, n) == hst).all()
    finally:
        for d in (d_pos, d_off, d_st, d_mv):
            d.free()


def test_game_state_legal_moves(engine):
    g = dchess.GameState("Alice", "Bob", engine)
    lm = g.legal_moves()
    assert len(lm) == 20
    for frm, to in lm:
        g.validate_move(frm, to)  # raises on a rejected move
    want = O.fast_gen_moves(O.Pos(), O.REF).tolist()
    assert [dchess.move_pack(f.x, f.y, t.x, t.y) for f, t in lm] == want
