"""GPU tests: every rules kernel under the board's symmetries (tests/symmetry.py).

  F  colour flip  (s ^ 56, colours and the side to move change, castle bits swap)
  M  file mirror  (s ^ 7; castle == 0 only: rights are cleared first, never skipped)
  R  = F o M      (s ^ 63)

The kernels are written per direction and per side (pawn_attacks<SIDE>, the
eight knight and king shifts with their file masks, one ray per direction,
lsb for one half of a line and msb for the other, every FIDE routine
instantiated once per side to move), and every other pin of the suite was
written beside them, White to move.  Here the call under test is always on
T(x), and the expected side is the existing reference's answer for x -- a
golden, a published table, oracle_lib or a model -- mapped through T; the GPU's
own answer for x is never the expected side.  tests/test_symmetry_model.py
checks on the CPU that those references are themselves invariant, so a
mismatch here is a one-sided kernel bug.

Digests, dc_gen_games, the state hash, history notation, SAN text and
signatures are not invariant by construction and are left out."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import dchess
import fide_positions as FP
import fide_replay_batches as FB
import oracle_lib as O
import outcome_model as OM
import san_model as S
import san_resolve_model as SR
import starts_batches as SB
import symmetry as Y
import test_gpu_final_parent_sums as PARSUM
import test_gpu_front_dedup as DEDUP
import test_gpu_legal_moves as LEGAL
import test_gpu_ref as REFT
from symmetry import F, M, R

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OG = json.load(open(os.path.join(GOLD, "oracle_golden.json")))
REF_D6 = json.load(open(os.path.join(GOLD, "ref_d6.json")))["positions"]
REF_DEEP = json.load(open(os.path.join(GOLD, "ref_deep.json")))
FX = json.load(open(os.path.join(GOLD, "perft_stats.json")))
REF, FIDE = dchess.RULES_REF, dchess.RULES_FIDE
SUITE = ["kiwipete", "pos3", "pos4", "pos5", "pos6", "startpos"]
W = 258
PAIRS = np.arange(4096, dtype=np.uint16)
TS = pytest.mark.parametrize("T", Y.ALL, ids=repr)


def _lib():
    L = dchess.lib()
    L.dc_test_perft_last_front.argtypes = [C.c_void_p]
    L.dc_test_front_dedup_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.dc_test_perft_stats_level_cap.argtypes = [C.c_void_p, C.c_uint64]
    L.dc_test_perft_stats_last_exact.argtypes = [C.c_void_p]
    L.dc_test_outcome_chunk_games.argtypes, L.dc_test_outcome_chunk_games.restype = [C.c_void_p, C.c_uint32], C.c_int
    return L


def front(e):
    return _lib().dc_test_perft_last_front(e.ctx)


def dedup_stats(e):
    out = (C.c_uint64 * 3)()
    assert _lib().dc_test_front_dedup_stats(e.ctx, out) == 0
    return tuple(int(x) for x in out)


def image(T, p):
    """(the position T takes, its image as a dc_pos record): M and R take p without its rights."""
    x = p if T is F else Y.without_rights(p)
    return x, SB.dpos(T.pos(x))


def as_dict(rm, div):
    return {int(m): int(v) for m, v in zip(rm, div)}


def int_keys(d):
    return {int(k): int(v) for k, v in d.items()}


def suite_pos(name):
    return O.Pos.from_fen(OG["perft_fide"][name]["fen"])


@functools.lru_cache(maxsize=None)
def oracle_perft(name, cleared, depth):
    """fast_perft of a suite position (or of it without its rights), computed once."""
    p = suite_pos(name)
    tot, div, rm = O.fast_perft(Y.without_rights(p) if cleared else p, depth, O.FIDE)
    return tot, as_dict(rm, div)


# ================================================= a. REF perft through the front end
@TS
@pytest.mark.parametrize("name", sorted(REF_D6))
def test_ref_d6_boards(engine, name, T):
    """The 16 boards of golden/ref_d6.json: perft(T(p), 6) is the golden with its
    divide keys mapped, unsharded (pos6 declined by the front end, the others
    taken) and as eight strided ply-3 shards."""
    e = REF_D6[name]
    p = SB.dpos(T.pos(O.Pos(np.array(e["cells"], np.int8), e["stm"], 0, -1)))
    want = T.divide(int_keys(e["divide"]))
    tot, div, rm = engine.perft(p, 6)
    assert tot == e["total"]
    assert as_dict(rm, div) == want
    assert front(engine) == (0 if name == "pos6" else 1)
    acc, t = {}, 0
    for k in range(8):
        st, sd, srm = engine.perft_shard(p, 6, 3, k, 8)
        t += st
        for m, v in zip(srm, sd):
            acc[int(m)] = acc.get(int(m), 0) + int(v)
    assert t == e["total"]
    assert {m: v for m, v in acc.items() if v} == {m: v for m, v in want.items() if v}


@TS
@pytest.mark.parametrize("depth", [5, 6, 7])
def test_ref_startpos(engine, depth, T):
    g = OG["perft_ref"]["startpos"][str(depth)]
    _, p = image(T, Y.without_rights(O.Pos()))
    tot, div, rm = engine.perft(p, depth)
    assert tot == g["total"]
    assert as_dict(rm, div) == T.divide(int_keys(g["divide"]))
    if depth == 7:
        assert front(engine) == 1
        assert dedup_stats(engine) == (197742, 72131, 125611)


def test_ref_startpos_depth8_flipped(engine):
    g = REF_DEEP["startpos_d8"]
    tot, div, rm = engine.perft(SB.dpos(F.pos(O.Pos())), 8)
    assert tot == g["total"]
    assert as_dict(rm, div) == F.divide(int_keys(g["divide"]))


SMALL_ROOTS = {"pawns_w": DEDUP.SMALL["pawns_w"][0], "pawns_b": DEDUP.SMALL["pawns_b"][0],
               "knight_w": DEDUP.SMALL["knight_w"][0], "many_w": PARSUM.MANY_W, "short": PARSUM.SHORT}


@TS
@pytest.mark.parametrize("name", sorted(SMALL_ROOTS))
def test_ref_small_roots_depth7(engine, name, T):
    """The oracle's perft(7) of the original, taken once and mapped; the dedup's
    owners are the original's distinct ply-4 boards."""
    fen = SMALL_ROOTS[name]
    want_tot, want_div = DEDUP._oracle(fen, 7)
    nodes, distinct = PARSUM._shape(fen)[:2] if name in ("many_w", "short") else DEDUP._levels(fen, 4)[4]
    _, p = image(T, O.Pos.from_fen(fen))
    tot, div, rm = engine.perft(p, 7)
    assert tot == want_tot
    assert as_dict(rm, div) == T.divide(want_div)
    assert front(engine) == 1
    assert dedup_stats(engine) == (nodes, distinct, nodes - distinct)


def test_ref_repeat_device_flipped_startpos(engine):
    g = OG["perft_ref"]["startpos"]["7"]
    p = SB.dpos(F.pos(O.Pos()))
    want = F.divide(int_keys(g["divide"]))
    runs = 9  # the 8-run batch graph and one single run
    buf = engine.alloc(runs * W * 8)
    try:
        _, _, rm = engine.perft(p, 7)
        assert sorted(int(m) for m in rm) == sorted(want)
        engine.perft_repeat_device(p, 7, 3, 0, 1, runs, buf)
        engine.synchronize()
        res = buf.download(np.uint64, runs * W).reshape(runs, W)
    finally:
        buf.free()
    assert (res[:, 256] == len(rm)).all()  # n_root, no overflow bit
    assert (res[:, 257] == g["total"]).all()
    assert (res[:, :len(rm)] == np.array([want[int(m)] for m in rm], np.uint64)).all() and not res[:, len(rm):256].any()


# ============================ b. FIDE perft from Black's side and from the other wing
@pytest.mark.parametrize("name", SUITE)
def test_fide_suite_flipped_published(engine, name):
    e = OG["perft_fide"][name]
    p = SB.dpos(F.pos(suite_pos(name)))
    for d in range(1, 6):
        tot, div, rm = engine.perft(p, d, rules=FIDE)
        assert tot == e["perft"][str(d)], d
        if d <= 3:
            assert as_dict(rm, div) == F.divide(oracle_perft(name, False, d)[1]), d


@pytest.mark.parametrize("name,depth", [("startpos", 7), ("pos3", 7), ("pos4", 6)])
def test_fide_deep_flipped_published(engine, name, depth):
    """pos4 at depth 6 is the published "Position 4 mirrored" row: the same number."""
    want = OG["perft_fide"][name]["perft"][str(depth)]
    if name == "startpos":
        assert want == 3195901860
    assert engine.perft(SB.dpos(F.pos(suite_pos(name))), depth, rules=FIDE)[0] == want


@pytest.mark.parametrize("n_shards,split", [(3, 4), (2, 3)])
def test_fide_startpos_flipped_shards(engine, n_shards, split):
    p = SB.dpos(F.pos(O.Pos()))
    t = sum(engine.perft_shard(p, 6, split, k, n_shards, rules=FIDE)[0] for k in range(n_shards))
    assert t == OG["perft_fide"]["startpos"]["perft"]["6"]


@pytest.mark.parametrize("T", [M, R], ids=repr)
@pytest.mark.parametrize("name", SUITE)
def test_fide_suite_without_rights_mirrored(engine, name, T):
    _, p = image(T, suite_pos(name))
    for d in range(1, 5):
        want_tot, want_div = oracle_perft(name, True, d)
        tot, div, rm = engine.perft(p, d, rules=FIDE)
        assert tot == want_tot, d
        assert as_dict(rm, div) == T.divide(want_div), d


@pytest.mark.parametrize("depth", [1, 2, 3, 4, 5])
def test_fide_batch_black_to_move(engine, depth):
    """The six F-images as one batch, Black to move: the published totals, and per
    position the oracle's divide of the original, mapped (to depth 4; at depth 5
    the divide sums to the published total)."""
    pos = [SB.dpos(F.pos(suite_pos(k))) for k in SUITE]
    assert all(int(p["stm"]) == 1 for p in pos)
    tot, div, rm, rp = engine.perft_batch(pos, depth, rules=FIDE)
    assert [int(x) for x in tot] == [OG["perft_fide"][k]["perft"][str(depth)] for k in SUITE]
    k = 0
    for i, name in enumerate(SUITE):
        roots = F.divide(oracle_perft(name, False, min(depth, 4))[1])
        n = len(roots)
        assert (rp[k:k + n] == i).all()
        assert sorted(int(m) for m in rm[k:k + n]) == sorted(roots)
        if depth <= 4:
            assert as_dict(rm[k:k + n], div[k:k + n]) == roots
        assert int(div[k:k + n].sum()) == OG["perft_fide"][name]["perft"][str(depth)]
        k += n
    assert k == len(rm)


def test_fide_batch_repeat_device_black_to_move(engine):
    pos = [SB.dpos(F.pos(suite_pos(k))) for k in SUITE]
    want = [F.divide(oracle_perft(name, False, 4)[1]) for name in SUITE]
    runs = 10  # one 8-run batch graph and two single runs
    buf = engine.alloc(runs * W * 8)
    try:
        _, _, rm, rp = engine.perft_batch(pos, 4, rules=FIDE)
        engine.perft_batch_repeat_device(pos, 4, 3, runs, buf, rules=FIDE)
        engine.synchronize()
        res = buf.download(np.uint64, runs * W).reshape(runs, W)
    finally:
        buf.free()
    assert len(rm) == sum(len(w) for w in want)
    record = np.array([want[int(i)][int(m)] for m, i in zip(rm, rp)], np.uint64)
    for r in range(runs):
        assert int(res[r, 256]) == len(rm)
        assert int(res[r, 257]) == sum(OG["perft_fide"][k]["perft"]["4"] for k in SUITE)
        assert (res[r, :len(rm)] == record).all() and not res[r, len(rm):256].any()


# ================================================================== c. perft_stats
def check_stats(engine, T, fen, depth, rules, e):
    x, p = image(T, O.Pos.from_fen(fen))
    tot, rows, rm = engine.perft_stats(p, depth, rules)
    assert tot.tolist() == e["totals"], (depth, tot.tolist(), e["totals"])
    if "rows" in e:
        want = T.divide({int(m): [int(v) for v in r] for m, r in zip(e["moves"], e["rows"])})
        assert {int(m): [int(v) for v in r] for m, r in zip(rm, rows)} == want, depth


@pytest.mark.parametrize("name", sorted(FX["fide_suite"]))
def test_stats_suite_flipped(engine, name):
    e = FX["fide_suite"][name]
    for d, ent in sorted(e["depths"].items()):
        check_stats(engine, F, e["fen"], int(d), FIDE, ent)


@pytest.mark.parametrize("i", range(len(FX["fide_small"])))
def test_stats_small_positions(engine, i):
    """Under F; under M and R the entries whose FEN names no rights."""
    e = FX["fide_small"][i]
    maps = Y.ALL if O.Pos.from_fen(e["fen"]).castle == 0 else (F,)
    for T in maps:
        for d in ("1", "2", "3"):
            assert "rows" in e["depths"][d]
            check_stats(engine, T, e["fen"], int(d), FIDE, e["depths"][d])


def test_stats_small_positions_cover_the_mirror():
    assert sum(O.Pos.from_fen(e["fen"]).castle == 0 for e in FX["fide_small"]) >= 5


def test_stats_ref_suite_flipped(engine):
    for name, e in FX["ref_suite"].items():
        for d, ent in sorted(e["depths"].items()):
            check_stats(engine, F, e["fen"], int(d), REF, ent)


def test_stats_forced_exact_rerun_flipped(engine):
    """F(kiwipete) at depth 4 as three shards with a level capacity of 1,000 nodes:
    every shard reruns in exact mode and they sum to the fixture."""
    L = _lib()
    e = FX["fide_suite"]["kiwipete"]
    p = SB.dpos(F.pos(O.Pos.from_fen(e["fen"])))
    roots = sorted(F.divide(oracle_perft("kiwipete", False, 1)[1]))
    assert L.dc_test_perft_stats_level_cap(engine.ctx, 1000) == dchess.SUCCESS
    try:
        total = np.zeros(dchess.PS_COUNT, np.uint64)
        for s in range(3):
            tot, rows, rm = engine.perft_stats(p, 4, FIDE, split_depth=2, shard=s, n_shards=3)
            assert L.dc_test_perft_stats_last_exact(engine.ctx) == 1
            assert sorted(int(m) for m in rm) == roots
            assert rows.sum(axis=0, dtype=np.uint64).tolist() == tot.tolist()
            total += tot
    finally:
        L.dc_test_perft_stats_level_cap(engine.ctx, 0)
    assert total.tolist() == e["depths"]["4"]["totals"]


# ========================================================== d. per-position calls
def junk_positions():
    """Six random boards of 24 pieces, kind 6 (OTHER) among them, either side to move."""
    rng = np.random.default_rng(5)
    out = []
    for _ in range(6):
        cells = np.full(64, -1, np.int8)
        sq = rng.choice(64, 24, replace=False)
        cells[sq] = rng.integers(0, 2, 24) * 8 + rng.integers(0, 7, 24)
        assert (cells & 7 == 6).any()
        out += [O.Pos(cells, stm, 0, -1) for stm in (0, 1)]
    return out


@functools.lru_cache(maxsize=None)
def position_sets(rules):
    if rules == FIDE:
        return tuple(FP.position_set()) + (O.Pos.from_fen(LEGAL.FEN_218),)
    return tuple(REFT._positions(16, 11)) + tuple(junk_positions())


def status_of(p, legal, rules):
    st = dchess.ST_NO_MOVES if len(legal) == 0 else 0
    if rules == FIDE:
        st |= (dchess.ST_CHECK if OM.in_check(p) else 0) | (dchess.ST_DEAD if OM.dead(p) else 0)
    return st


class Set:
    """Per T: the positions the map takes (xs), their images (dc_pos), and the oracle's
    answers for xs: legal lists, all-pairs verdicts, status."""

    def __init__(self, rules, T):
        self.xs = [p if T in (Y.I, F) else Y.without_rights(p) for p in position_sets(rules)]
        self.pos = SB.pos_array([T.pos(x) for x in self.xs])
        self.lists = [O.fast_gen_moves(x, rules) for x in self.xs]
        self.status = np.array([status_of(x, l, rules) for x, l in zip(self.xs, self.lists)], np.uint8)

    def verdicts(self, rules, i):
        x = self.xs[i]
        return O.fast_verdicts_all(x, O.FIDE) if rules == FIDE else O.ref_verdicts_all(x.cells, x.stm)


@functools.lru_cache(maxsize=None)
def the_set(rules, T):
    return Set(rules, T)


@TS
@pytest.mark.parametrize("rules", [REF, FIDE], ids=["ref", "fide"])
def test_validate_all_pairs(engine, rules, T):
    s = the_set(rules, T)
    idx = T.words4096()  # (the oracles' tables are indexed 64 * from + to: the same xor maps the index)
    by_index = (PAIRS >> 6) | ((PAIRS & 63) << 6)
    for lo in range(0, len(s.xs), 128):
        hi = min(lo + 128, len(s.xs))
        got = engine.validate_batch(np.repeat(s.pos[lo:hi], 4096), np.tile(by_index, hi - lo), rules).reshape(-1, 4096)
        want = np.stack([s.verdicts(rules, i) for i in range(lo, hi)])
        bad = np.argwhere(got[:, idx] != want)
        assert len(bad) == 0, [(T, lo + int(r), hex(int(c)), int(got[r, idx[c]]), int(want[r, c])) for r, c in bad[:5]]


@TS
def test_validate_promotion_codes(engine, T):
    """Every promotion code 0..7 on the legal promotion pairs and on their images
    under F, M and R in the same position (the twins), against the oracle's validate."""
    s = the_set(FIDE, T)
    pos, words, want = [], [], []
    for i, (x, legal) in enumerate(zip(s.xs, s.lists)):
        pairs = sorted({int(m) & 0xFFF for m in legal if int(m) >> 12})
        twins = sorted({U.moves(w) for w in pairs for U in (Y.I,) + Y.ALL})
        for w in twins:
            for code in range(8):
                pos.append(i)
                words.append(w | (code << 12))
                want.append(O.fast_validate(x, w | (code << 12), O.FIDE))
    assert len(words) >= 2000 and want.count(O.OK) >= 200
    got = engine.validate_batch(s.pos[pos], T.moves(np.array(words, np.uint16)), FIDE)
    assert (got == np.array(want, np.uint8)).all()


@TS
@pytest.mark.parametrize("rules", [REF, FIDE], ids=["ref", "fide"])
def test_apply_every_legal_move(engine, rules, T):
    s = the_set(rules, T)
    par = np.repeat(np.arange(len(s.xs)), [len(l) for l in s.lists])
    mv = np.concatenate(s.lists).astype(np.uint16)
    kids, info = [], []
    for i, m in zip(par.tolist(), mv.tolist()):
        x = s.xs[i]
        kids.append(T.pos(O.fast_make(x, m, rules)))
        info.append((int(x.cells[m & 63]) & 7) | (8 if x.cells[(m >> 6) & 63] >= 0 else 0))
    want = SB.pos_array(kids)
    new, ver, got_info = engine.apply_batch(s.pos[par], T.moves(mv), rules)
    assert (ver == dchess.V_OK).all()
    for field in ("bb", "stm", "castle", "ep"):
        bad = np.flatnonzero((new[field] != want[field]).reshape(len(mv), -1).any(axis=1))
        assert len(bad) == 0, [(T, field, int(par[j]), hex(int(mv[j]))) for j in bad[:5]]
    assert (got_info == np.array(info, np.uint8)).all()


@pytest.mark.parametrize("size", [256, 257])
@pytest.mark.parametrize("rules", [REF, FIDE], ids=["ref", "fide"])
def test_legal_moves_four_images_adjacent(engine, rules, size):
    """x, F(x), M(x0) and R(x0) in neighbouring lanes (one wave holds all four), the
    whole set in calls of `size` positions: offsets from the original's list
    lengths, the lists mapped and re-sorted, the status as it is."""
    maps = (Y.I,) + Y.ALL
    sets = [the_set(rules, T) for T in maps]
    n = len(sets[0].xs)
    pos = np.stack([s.pos for s in sets], axis=1).reshape(-1)
    lists = [T.canonical(T.moves(s.lists[i])) for i in range(n) for T, s in zip(maps, sets)]
    status = np.stack([s.status for s in sets], axis=1).reshape(-1)
    if rules == FIDE:
        assert max(len(l) for l in lists) == 218
        assert (status & dchess.ST_CHECK).any() and (status & dchess.ST_NO_MOVES).any() and (status & dchess.ST_DEAD).any()
    for lo in range(0, len(pos), size):
        hi = min(lo + size, len(pos))
        off, mv, st = engine.legal_moves(pos[lo:hi], rules)
        want_off = np.zeros(hi - lo + 1, np.int64)
        want_off[1:] = np.cumsum([len(l) for l in lists[lo:hi]])
        assert (off == want_off).all(), lo
        want_mv = np.concatenate(lists[lo:hi]) if want_off[-1] else np.zeros(0, np.uint16)
        bad = np.flatnonzero(mv != want_mv)
        assert len(bad) == 0, (lo, [(int(j), hex(int(mv[j])), hex(int(want_mv[j]))) for j in bad[:5]])
        assert (st == status[lo:hi]).all(), lo


# ============================================== e. replay, adjudication, SAN, resolver
def test_the_batch_has_its_shape():
    """Among the unmapped columns: every result, both castles of both colours, an
    en-passant capture, every promotion code, SAN with a file, a rank and both, and
    resolver words of both kinds."""
    s = Y.batch_shape()
    assert s["results"] == set(range(dchess.GO_COUNT))
    assert s["castles"] == {(0, "k"), (0, "q"), (1, "k"), (1, "q")}
    assert s["ep"] >= 1 and s["promos"] == {1, 2, 3, 4}
    assert {S.FILE, S.RANK, S.FILE | S.RANK} <= s["san"]
    assert {SR.NOMATCH, SR.AMBIGUOUS} <= s["words"]
    c = Y.columns()
    assert all(c.T[g] is not c.T[g + 1] or c.T[g] is Y.I for g in range(c.n - 1))  # neighbouring lanes differ


def check_replay(c, out, san, bm, counts, st, finals):
    for field, want in (("result", c.result), ("end_ply", c.end_ply), ("repeats", c.repeats), ("halfmove", c.halfmove)):
        bad = np.flatnonzero(out[field] != want)
        assert len(bad) == 0, (field, [(int(g), c.T[g], int(out[field][g]), int(want[g])) for g in bad[:5]])
    assert (bm == c.bitmap).all()
    if san is not None:
        bad = np.argwhere(san != c.san)
        assert len(bad) == 0, [(int(p), int(g), c.T[g], int(san[p, g]), int(c.san[p, g])) for p, g in bad[:5]]
    bad = np.flatnonzero(~SB.same_pos(finals, c.finals).all(axis=1))
    assert len(bad) == 0, [(int(g), c.T[g]) for g in bad[:5]]
    assert counts.tolist() == c.counts.tolist()
    assert (st["validated"], st["accepted"], st["rejected"]) == (c.validated, c.accepted, c.validated - c.accepted)


@pytest.fixture()
def small_chunks(engine):
    """Chunks of 256 games, so that the batch spans several launches."""
    hook = _lib().dc_test_outcome_chunk_games
    assert hook(engine.ctx, 256) == 0
    yield
    assert hook(engine.ctx, 177664) == 0


def test_replay_outcome_starts(engine, small_chunks):
    c = Y.columns()
    out, bm, dg, counts, st, finals = engine.replay_outcome_starts(c.moves, c.dstarts, c.clocks)
    check_replay(c, out, None, bm, counts, st, finals)


def test_replay_san_starts(engine, small_chunks):
    c = Y.columns()
    out, san, bm, dg, counts, st, finals = engine.replay_san_starts(c.moves, c.dstarts, c.clocks)
    check_replay(c, out, san, bm, counts, st, finals)


def test_replay_starts_device_forms(engine, small_chunks):
    c = Y.columns()
    n, n_plies = c.n, c.moves.shape[0]
    words = (n + 63) // 64
    sizes = (c.moves.nbytes, 40 * n, 2 * n, 8 * n, n * n_plies, 8 * words * n_plies, 40 * n)
    d_mv, d_st, d_hm, d_out, d_san, d_bm, d_fin = bufs = [engine.alloc(k) for k in sizes]
    try:
        d_mv.upload(c.moves)
        d_st.upload(c.dstarts)
        d_hm.upload(c.clocks)

        def fetch():
            return (d_out.download(dchess.OUTCOME_DTYPE, n), d_bm.download(np.uint64, words * n_plies).reshape(n_plies, words),
                    d_fin.download(dchess.POS_DTYPE, n))

        counts, st = engine.replay_outcome_starts_device(d_mv, n, n_plies, d_out, d_bm, None, d_st, d_hm, d_fin)
        out, bm, finals = fetch()
        check_replay(c, out, None, bm, counts, st, finals)
        counts, st = engine.replay_san_starts_device(d_mv, n, n_plies, d_out, d_san, d_bm, None, d_st, d_hm, d_fin)
        out, bm, finals = fetch()
        check_replay(c, out, d_san.download(np.uint8, n * n_plies).reshape(n_plies, n), bm, counts, st, finals)
    finally:
        for b in bufs:
            b.free()


def test_resolve_san_starts(engine):
    c = Y.columns()
    moves, first_bad, counts, finals = engine.resolve_san_starts(c.tokens, c.dstarts)
    bad = np.argwhere(moves != c.words)
    assert len(bad) == 0, [(int(p), int(g), c.T[g], hex(int(moves[p, g])), hex(int(c.words[p, g]))) for p, g in bad[:5]]
    assert (first_bad == c.first_bad).all() and counts.tolist() == c.resolve_counts.tolist()
    bad = np.flatnonzero(~SB.same_pos(finals, c.resolved_finals).all(axis=1))
    assert len(bad) == 0, [(int(g), c.T[g]) for g in bad[:5]]
    flagged = (c.words & 0x8000) != 0
    assert (moves[flagged] == np.stack([b.words for b in c.base], axis=1)[flagged]).all()  # flagged words: as they are


@TS
def test_dc_replay_fide_shared_start(engine, T):
    """dc_replay from T(start) on T(moves): the oracle's bitmap and counters for the original."""
    cs = FB.custom_starts()
    played = 0
    for i in (0, 4, 9, 13, 21, len(cs) - 5):
        x, start = image(T, cs[i][1])
        mv = FB.games_from(i)
        bm, _, st = O.fast_replay(mv, rules=O.FIDE, start=x)
        gbm, _, gst = engine.replay(T.moves(np.array(mv)), rules=FIDE, start=start, want_digests=False)
        assert (gbm == bm).all(), (T, i)
        assert [gst[k] for k in ("validated", "accepted", "rejected")] == [int(v) for v in st[:3]], (T, i)
        played += int(st[1])
    assert played >= 4000


def ref_starts():
    mid = REFT._positions(1, 44)[0]
    rng = np.random.default_rng(9)
    cells = np.full(64, -1, np.int8)
    sq = rng.choice(64, 26, replace=False)
    cells[sq] = rng.integers(0, 2, 26) * 8 + rng.integers(0, 7, 26)  # includes kind 6 (OTHER)
    return {"midgame_black": O.Pos(mid.cells, 1, 0, -1), "odd_pieces": O.Pos(cells, 1, 0, -1)}


def ref_info(start, mv):
    """dc_replay_info's bytes of a REF batch, move by move through the literal
    restatement: the moved kind | 8 where the target held a piece, 0xFF where the word is not accepted."""
    info = np.full(mv.shape, 0xFF, np.uint8)
    for g in range(mv.shape[1]):
        cells, stm = start.cells.copy(), start.stm
        for ply, m in enumerate(mv[:, g].tolist()):
            f, t = m & 63, (m >> 6) & 63
            if m & 0x8000 or O.ref_validate(cells, stm, f >> 3, f & 7, t >> 3, t & 7) != O.OK:
                continue
            info[ply, g] = (int(cells[f]) & 7) | (8 if cells[t] >= 0 else 0)
            cells[t], cells[f] = cells[f], -1
            stm ^= 1
    return info


@TS
@pytest.mark.parametrize("kind", ["midgame_black", "odd_pieces"])
def test_dc_replay_ref_and_info(engine, kind, T):
    start = ref_starts()[kind]
    mv, bm, _, validated, accepted = REFT._replay_from(start, 100, 37, 5)
    assert accepted > 500
    tstart, tmv = SB.dpos(T.pos(start)), T.moves(mv)
    gbm, _, st = engine.replay(tmv, start=tstart, want_digests=False)
    assert (gbm == bm).all() and (st["validated"], st["accepted"]) == (validated, accepted)
    gbm, _, info, st = engine.replay_info(tmv, start=tstart, want_digests=False)
    assert (gbm == bm).all() and (st["validated"], st["accepted"]) == (validated, accepted)
    assert (info == ref_info(start, mv)).all()
