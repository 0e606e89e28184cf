"""GPU tests of dc_perft_stats / dc_perft_stats_shard: the published perft
tables' columns (captures, en passant, castles, promotions, checks, discovered
and double checks, mates) and, under REF, captures and king captures.

Expected values come from tests/golden/perft_stats.json (the fastcpu oracle's
moves, classified by the mailbox attack walk of tests/cpp/perft_stats_oracle.cpp;
the generator asserts the published tables before it writes), and, fixture-free,
from Engine.legal_moves / apply_batch over positions of seeded games."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import dchess
from dchess import (PS_CAPTURES, PS_CHECKMATES, PS_CHECKS, PS_COUNT, PS_KING_CAPTURES, PS_NODES, PS_STALEMATES)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FX = json.load(open(os.path.join(HERE, "golden", "perft_stats.json")))
OG = json.load(open(os.path.join(HERE, "golden", "oracle_golden.json")))
REF, FIDE = dchess.RULES_REF, dchess.RULES_FIDE
SUITE = sorted(FX["fide_suite"])
REF_ONLY = (PS_NODES, PS_CAPTURES, PS_KING_CAPTURES)


def by_move(moves, rows):
    return {int(m): [int(v) for v in r] for m, r in zip(moves, rows)}


def check_entry(engine, pos, depth, rules, e):
    tot, rows, rm = engine.perft_stats(pos, depth, rules)
    assert tot.tolist() == e["totals"], (depth, tot.tolist(), e["totals"])
    assert rows.sum(axis=0, dtype=np.uint64).tolist() == tot.tolist()
    if "rows" in e:
        assert by_move(rm, rows) == by_move(e["moves"], e["rows"]), depth
    return tot, rows, rm


# --------------------------------------------------------------- the fixture
@pytest.mark.parametrize("name", SUITE)
def test_suite_totals(engine, name):
    """Every row of the published tables (and the depths below it)."""
    e = FX["fide_suite"][name]
    pos = dchess.pos_from_fen(e["fen"])
    assert len(e["depths"]) >= 4
    for d, ent in sorted(e["depths"].items()):
        check_entry(engine, pos, int(d), FIDE, ent)


@pytest.mark.parametrize("i", range(len(FX["fide_small"])))
def test_small_positions_rows(engine, i):
    """The rare branches (stalemate, a castle that checks, an en-passant
    discovery, double checks, promotions) with every per-root row."""
    e = FX["fide_small"][i]
    pos = dchess.pos_from_fen(e["fen"])
    for d in ("1", "2", "3"):
        assert "rows" in e["depths"][d]
        check_entry(engine, pos, int(d), FIDE, e["depths"][d])


@pytest.mark.parametrize("name", ["kiwipete", "pos4"])
def test_suite_rows_depth3(engine, name):
    e = FX["fide_suite"][name]
    assert "rows" in e["depths"]["3"]
    check_entry(engine, dchess.pos_from_fen(e["fen"]), 3, FIDE, e["depths"]["3"])


@pytest.mark.parametrize("name,depth,rules", [("kiwipete", 3, FIDE), ("startpos", 4, FIDE), ("pos4", 3, FIDE),
                                               ("startpos", 4, REF), ("kiwipete", 3, REF)])
def test_rows_consistent_with_perft(engine, name, depth, rules):
    pos = dchess.pos_from_fen(FX["fide_suite"][name]["fen"])
    tot, rows, rm = engine.perft_stats(pos, depth, rules)
    ptot, div, prm = engine.perft(pos, depth, rules)
    assert rm.tolist() == prm.tolist()
    assert rows[:, PS_NODES].tolist() == div.tolist()
    assert int(tot[PS_NODES]) == ptot
    assert rows.sum(axis=0, dtype=np.uint64).tolist() == tot.tolist()


# -------------------------------------------------------------------- shards
@pytest.mark.parametrize("name,depth,split,n_shards", [("kiwipete", 4, 2, 3), ("pos4", 3, 1, 64)])
def test_shards_sum_to_the_whole(engine, name, depth, split, n_shards):
    """pos4 has 6 root moves: at split_depth 1 most of the 64 shards are empty."""
    pos = dchess.pos_from_fen(FX["fide_suite"][name]["fen"])
    tot, rows, rm = engine.perft_stats(pos, depth, FIDE)
    assert tot.tolist() == FX["fide_suite"][name]["depths"][str(depth)]["totals"]
    stot = np.zeros(PS_COUNT, np.uint64)
    srows = np.zeros_like(rows)
    empty = 0
    for s in range(n_shards):
        t, r, m = engine.perft_stats(pos, depth, FIDE, split_depth=split, shard=s, n_shards=n_shards)
        assert m.tolist() == rm.tolist()
        assert r.sum(axis=0, dtype=np.uint64).tolist() == t.tolist()
        stot += t
        srows += r
        empty += int(t[PS_NODES] == 0)
    assert stot.tolist() == tot.tolist()
    assert (srows == rows).all()
    if n_shards == 64:
        assert empty >= 64 - 6


# ----------------------------------------------------------------------- REF
def test_ref_pins_and_rows(engine):
    for name, e in FX["ref_suite"].items():
        pos = dchess.pos_from_fen(e["fen"])
        for d, ent in sorted(e["depths"].items()):
            tot, _, _ = check_entry(engine, pos, int(d), REF, ent)
            assert not any(int(tot[k]) for k in range(PS_COUNT) if k not in REF_ONLY)
    assert "rows" in FX["ref_suite"]["startpos"]["depths"]["3"]
    assert FX["ref_suite"]["startpos"]["depths"]["5"]["totals"][PS_KING_CAPTURES] == 461


def test_ref_random_positions(engine):
    assert len(FX["ref_random"]) == 8
    for e in FX["ref_random"]:
        g = OG["perft_ref"]["random_positions"][e["index"]]
        pos = dchess.pos_from_cells(np.array(g["cells"], np.int8), g["stm"])
        for d in ("1", "2", "3"):
            tot, rows, _ = check_entry(engine, pos, int(d), REF, e["depths"][d])
            assert not any(int(rows[:, k].sum()) for k in range(PS_COUNT) if k not in REF_ONLY)


# ------------------------------------------- fixture-free: the existing paths
def test_depth1_matches_legal_moves_and_apply(engine):
    """Depth-1 NODES, CAPTURES, CHECKS, CHECKMATES and STALEMATES of ~200 FIDE
    positions from seeded games against Engine.legal_moves of the children that
    Engine.apply_batch makes."""
    n, plies = 200, 100
    mv = engine.gen_games(0xC0FFEE, 0, n, plies, 0, rules=FIDE)
    stop = np.random.default_rng(5).integers(0, plies, n)
    cur = np.repeat(np.array([dchess.startpos()], dchess.POS_DTYPE), n)
    cur["castle"] = 15
    snap = cur.copy()
    for ply in range(plies):
        at = stop == ply
        snap[at] = cur[at]
        cur, _, _ = engine.apply_batch(cur, mv[ply], FIDE)  # (a sentinel move is rejected: the game stays over)
    off, moves, _ = engine.legal_moves(snap, FIDE)
    par = np.repeat(np.arange(n), np.diff(off.astype(np.int64)))
    child, ver, info = engine.apply_batch(snap[par], moves, FIDE)
    assert (ver == dchess.V_OK).all()
    _, _, st = engine.legal_moves(child, FIDE)
    chk = (st & dchess.ST_CHECK) != 0
    nom = (st & dchess.ST_NO_MOVES) != 0
    to = (moves >> 6) & 63
    ep = ((info & 7) == 0) & (snap["ep"][par] >= 0) & (to == snap["ep"][par].astype(np.int64))
    cap = ((info & 8) != 0) | ep
    seen = np.zeros(PS_COUNT, np.int64)
    for g in range(n):
        tot, rows, rm = engine.perft_stats(snap[g], 1, FIDE)
        s = slice(int(off[g]), int(off[g + 1]))
        want = {PS_NODES: s.stop - s.start, PS_CAPTURES: int(cap[s].sum()), PS_CHECKS: int(chk[s].sum()),
                PS_CHECKMATES: int((chk[s] & nom[s]).sum()), PS_STALEMATES: int((~chk[s] & nom[s]).sum())}
        for k, v in want.items():
            assert int(tot[k]) == v, (g, dchess.PS_NAMES[k], int(tot[k]), v)
        assert sorted(rm.tolist()) == sorted(moves[s].tolist())
        # ... and per root move
        order = {int(m): j for j, m in enumerate(moves[s].tolist())}
        for m, r in zip(rm.tolist(), rows):
            j = s.start + order[m]
            assert (int(r[PS_CAPTURES]), int(r[PS_CHECKS])) == (int(cap[j]), int(chk[j])), (g, m)
        seen += tot.astype(np.int64)
    assert seen[PS_NODES] > 2000 and seen[PS_CAPTURES] > 100 and seen[PS_CHECKS] > 50  # the sample is not trivial


def test_kingless_side_is_never_in_check(engine):
    cells = np.full(64, dchess.CELL_EMPTY, np.int8)
    cells[4], cells[0], cells[3] = 5, 3, 4          # white K e1, R a1, Q d1
    cells[48], cells[51], cells[62] = 8, 8, 8 + 1    # black pawns a7, d7, knight g8: no king
    pos = dchess.pos_from_cells(cells, 0)
    for d in (1, 2, 3):
        tot, rows, _ = engine.perft_stats(pos, d, FIDE)
        assert int(tot[PS_NODES]) == engine.perft(pos, d, FIDE)[0] > 0
        if d & 1:  # white moved last: black, kingless, is never in check
            assert int(tot[PS_CHECKS]) == int(tot[PS_CHECKMATES]) == 0
            assert int(tot[dchess.PS_DISCOVERED]) == int(tot[dchess.PS_DOUBLE]) == 0


# ------------------------------------------------------ depth 0, 1 and errors
def test_depth0_and_depth1(engine):
    pos = dchess.pos_from_fen(FX["fide_suite"]["kiwipete"]["fen"])
    for rules in (REF, FIDE):
        tot, rows, rm = engine.perft_stats(pos, 0, rules)
        assert tot.tolist() == [1] + [0] * (PS_COUNT - 1) and len(rows) == 0 and len(rm) == 0
        tot, rows, rm = engine.perft_stats(pos, 0, rules, split_depth=1, shard=1, n_shards=2)
        assert tot.tolist() == [0] * PS_COUNT and len(rm) == 0
    # depth 1 classifies the root's own moves, one row each
    tot, rows, rm = engine.perft_stats(pos, 1, FIDE)
    assert tot.tolist() == FX["fide_suite"]["kiwipete"]["depths"]["1"]["totals"]
    assert rows[:, PS_NODES].tolist() == [1] * 48
    assert rm.tolist() == engine.perft(pos, 1, FIDE)[2].tolist()
    assert int(rows[:, dchess.PS_CASTLES].sum()) == 2 and int(rows[:, PS_CAPTURES].sum()) == 8
    # ... and shard 0 holds them all
    t0, r0, m0 = engine.perft_stats(pos, 1, FIDE, split_depth=1, shard=0, n_shards=2)
    t1, r1, m1 = engine.perft_stats(pos, 1, FIDE, split_depth=1, shard=1, n_shards=2)
    assert t0.tolist() == tot.tolist() and (r0 == rows).all() and not t1.any() and not r1.any()
    assert m0.tolist() == m1.tolist() == rm.tolist()


def test_argument_errors(engine):
    L = dchess.lib()
    pos = np.array([dchess.startpos()], dchess.POS_DTYPE)
    tot = np.zeros(PS_COUNT, np.uint64)
    nr = C.c_uint32()

    def call(rules=FIDE, p=pos, depth=2, split=1, shard=0, n_shards=1, totals=tot):
        return L.dc_perft_stats_shard(engine.ctx, rules, dchess._ptr(p), depth, split, shard, n_shards,
                                      dchess._ptr(totals), None, None, C.byref(nr))

    assert call() == dchess.SUCCESS and int(tot[PS_NODES]) == 400
    assert call(rules=2) == dchess.EINVAL
    assert call(p=None) == dchess.EINVAL
    assert call(totals=None) == dchess.EINVAL
    assert call(shard=2, n_shards=2) == dchess.EINVAL
    assert call(n_shards=0) == dchess.EINVAL
    bad = pos.copy()
    bad["stm"] = 2
    assert call(p=bad) == dchess.EINVAL
    assert call(depth=13) == dchess.EUNSUPPORTED


# ------------------------------------------------------------------ profiling
def test_leaf_stats_is_reported(engine):
    pos = dchess.pos_from_fen(FX["fide_suite"]["kiwipete"]["fen"])
    engine.set_profiling(True)
    try:
        engine.reset_stats()
        tot, _, _ = engine.perft_stats(pos, 3, FIDE)
        ks = engine.kernel_stats("leaf_stats")
    finally:
        engine.set_profiling(False)
    assert ks["launches"] >= 1 and ks["units"] == int(tot[PS_NODES]) == 97862
    assert ks["total_ms"] > 0


# ---------------------------------------------------------------- exact rerun
@pytest.mark.parametrize("name,depth,rules,shards,cap", [("startpos", 5, FIDE, 1, 10000), ("kiwipete", 3, REF, 1, 1000),
                                                          ("kiwipete", 4, FIDE, 3, 1000)])
def test_forced_exact_rerun_gives_the_same(engine, name, depth, rules, shards, cap):
    """A level past its speculative capacity is flagged on the device and the
    run repeated in exact mode (host-sized levels): forced here by a capacity of
    `cap` nodes per level (dc_test_perft_stats_level_cap).  startpos: ply 3
    (8,902) fits and ply 4 (197,281) does not, so a level kernel's scan flags
    it; kiwipete: ply 2 (2,039) overflows in the top kernel, and the sharded
    case gathers its shard of ply 2 in exact mode."""
    L = dchess.lib()
    L.dc_test_perft_stats_level_cap.argtypes = [C.c_void_p, C.c_uint64]
    L.dc_test_perft_stats_last_exact.argtypes = [C.c_void_p]
    pos = dchess.pos_from_fen(FX["fide_suite"][name]["fen"])
    want = [engine.perft_stats(pos, depth, rules, split_depth=2, shard=s, n_shards=shards) for s in range(shards)]
    assert L.dc_test_perft_stats_last_exact(engine.ctx) == 0
    assert L.dc_test_perft_stats_level_cap(engine.ctx, cap) == dchess.SUCCESS
    try:
        for s in range(shards):
            tot, rows, rm = engine.perft_stats(pos, depth, rules, split_depth=2, shard=s, n_shards=shards)
            assert L.dc_test_perft_stats_last_exact(engine.ctx) == 1
            assert tot.tolist() == want[s][0].tolist() and (rows == want[s][1]).all()
            assert rm.tolist() == want[s][2].tolist()
    finally:
        L.dc_test_perft_stats_level_cap(engine.ctx, 0)
    key = "fide_suite" if rules == FIDE else "ref_suite"
    assert sum(w[0] for w in want).tolist() == FX[key][name]["depths"][str(depth)]["totals"]
    engine.perft_stats(pos, 2, rules)
    assert L.dc_test_perft_stats_last_exact(engine.ctx) == 0
