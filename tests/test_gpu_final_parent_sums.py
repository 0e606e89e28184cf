"""GPU tests: the per-parent sums of REF perft(7)'s deduplicated final stage
(k_count3c<.., DEDUP> with c2c_group<.., PARSUM>).

The final stage sums a group's leaves per parent in LDS (32-bit adds into
sums[parent's thread]); at the group's end each wave reduces the runs of
parents that share a grandparent and adds one total per run into gp_total.
The roots below are chosen for the shapes at which that can go wrong: many
run boundaries in a wave, a block that takes a second group (its sums reused),
a short last group, and parents with many moves.  Expected values come from the
CPU oracle (oracle_lib) at run time or from tests/golden; the shape of each
root (owners, move words) is computed from the oracle's distinct-board walk
and asserted, so a root that no longer has the shape fails instead of passing
for nothing.

A "word" is one child of a distinct ply-4 board (an owner): the final stage
takes the words in groups of 256, on a grid of 1,024 blocks whose first group
is their own index."""
import ctypes as C
import json
import os
import threading

import numpy as np
import pytest

import dchess
import oracle_lib as O

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
OG = json.load(open(os.path.join(GOLD, "oracle_golden.json")))
W = 258
GROUP = 256
GRID = 1024

# 1. pawns and a king: 4.1 words per owner, so a group holds about 62 grandparents
MANY_W = "8/pppp4/8/6k1/8/PPPP4/8/8 w - - 0 1"
MANY_B = "8/8/pppp4/8/6K1/8/PPPP4/8 b - - 0 1"
# 2. reduced material, more than 2 x 256 x 1,024 words: every block takes a second group
BIG_W = "r3k3/ppp3pp/8/8/8/8/PPP3PP/R3K3 w - - 0 1"
BIG_B = "r3k3/ppp3pp/8/8/8/8/PPP3PP/R3K3 b - - 0 1"
# 3. fewer words than one round of the grid, and not a multiple of 256
SHORT = "r3k3/p6p/8/8/8/8/P6P/R3K3 w - - 0 1"
# 4. two queens and two rooks against a king: the parents are the heavy side's boards
HEAVY = "3qkq2/r6r/8/8/8/8/8/4K3 w - - 0 1"


def _lib():
    L = dchess.lib()
    L.dc_test_perft_last_front.argtypes = [C.c_void_p]
    L.dc_test_front_dedup_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    return L


def _front(e):
    return _lib().dc_test_perft_last_front(e.ctx)


def _stats(e):
    out = (C.c_uint64 * 3)()
    assert _lib().dc_test_front_dedup_stats(e.ctx, out) == 0
    return tuple(int(x) for x in out)


_SHAPE = {}


def _shape(fen):
    """(ply-4 nodes, distinct ply-4 boards, move words = the distinct boards'
    moves, the largest move count of one) from the oracle's walk, computed once."""
    if fen not in _SHAPE:
        p0 = O.Pos.from_fen(fen)
        cur = {p0.cells.tobytes(): (p0, 1)}
        for _ in range(4):
            nxt = {}
            for p, mult in cur.values():
                for m in O.fast_gen_moves(p):
                    q = O.fast_make(p, int(m))
                    k = q.cells.tobytes()
                    if k in nxt:
                        nxt[k] = (nxt[k][0], nxt[k][1] + mult)
                    else:
                        nxt[k] = (q, mult)
            cur = nxt
        counts = [len(O.fast_gen_moves(p)) for p, _ in cur.values()]
        _SHAPE[fen] = (sum(m for _, m in cur.values()), len(cur), sum(counts), max(counts))
    return _SHAPE[fen]


_ORACLE = {}


def _oracle(fen):
    if fen not in _ORACLE:
        tot, div, rm = O.fast_perft(O.Pos.from_fen(fen), 7)
        _ORACLE[fen] = (tot, {int(m): int(v) for m, v in zip(rm, div)})
    return _ORACLE[fen]


def _check(e, fen):
    """perft(7) on the deduplicating front path: total, divide and owner counts are the oracle's."""
    tot, div, rm = e.perft(dchess.pos_from_fen(fen), 7)
    want_tot, want_div = _oracle(fen)
    assert _front(e) == 1, fen
    assert tot == want_tot, fen
    assert {int(m): int(v) for m, v in zip(rm, div)} == want_div, fen
    nodes, distinct, _, _ = _shape(fen)
    assert _stats(e) == (nodes, distinct, nodes - distinct), fen
    return tot, div, rm


@pytest.mark.parametrize("fen", [MANY_W, MANY_B], ids=["white", "black"])
def test_many_grandparents_in_a_wave(engine, fen):
    """A few thousand words at about four per owner: a group spans 60 or more
    grandparents, so nearly every wave holds many runs (15 or so), and the
    level is several groups with a short last one."""
    nodes, distinct, words, most = _shape(fen)
    assert words >= 2000 and words * 60 <= distinct * GROUP, (words, distinct)
    assert most <= 8 and words % GROUP != 0
    for _ in range(2):  # the plain run, then the captured graph
        _check(engine, fen)


@pytest.mark.parametrize("fen", [BIG_W, BIG_B], ids=["white", "black"])
def test_block_takes_second_group(engine, fen):
    """More than 524,288 words: every block of the grid takes a second group
    and so reuses its sums.  The eight strided shards take the plain
    instantiation (per-tag histogram): their sum is a differential check."""
    nodes, distinct, words, _ = _shape(fen)
    assert words > 2 * GROUP * GRID and nodes < (1 << 20), (words, nodes)
    tot, div, rm = _check(engine, fen)
    acc, t = np.zeros_like(div), 0
    for k in range(8):
        st, sd, srm = engine.perft_shard(dchess.pos_from_fen(fen), 7, 3, k, 8)
        assert _front(engine) == 1
        assert _stats(engine)[0] == 0  # (a shard does not deduplicate)
        assert (srm == rm).all()
        acc += sd
        t += st
    assert t == tot and (acc == div).all()


def test_startpos(engine):
    """Startpos perft(7): 1,810,818 words, 7,074 groups, against the golden."""
    g = OG["perft_ref"]["startpos"]["7"]
    tot, div, rm = engine.perft(dchess.startpos(), 7)
    assert _front(engine) == 1
    assert tot == g["total"]
    assert {str(int(m)): int(v) for m, v in zip(rm, div)} == g["divide"]
    assert _stats(engine) == (197742, 72131, 197742 - 72131)


def test_short_last_group(engine):
    """Fewer words than one round of the grid (no block takes a second group)
    and a last group of 7 words: 249 of its lanes are empty slots."""
    _, _, words, _ = _shape(SHORT)
    assert words < GROUP * GRID and words % GROUP != 0, words
    assert words % GROUP == 7
    _check(engine, SHORT)


def test_heavy_parents(engine):
    """Parents of 29 to 83 moves (mean 60.6; 58 % have 60 or more), the side
    with two queens and two rooks to move; a parent's sum reaches 664.

    Sums of tens of thousands are out of the oracle's reach: they need both
    sides heavy, and perft(7) is about (root side's moves)^4 x (other side's)^3,
    2.8e12 leaves at 60 moves each, while no promotion exists under these rules
    to make a light root heavy further down.  This root has 361,293,751.

    The multi-window branch (more than 4,592 special children in a group) is not
    reached.  With a lone king on the other side there are no slider rays and
    no pawn-sensitive squares, so a parent's special children are its captures:
    counted with the oracle over all 178,711 parents, the 256 parents with the
    most captures have 769 between them.  A root that reaches the branch needs
    sliders or pawns on the light side too, which puts its perft(7) past 1e10
    leaves; the branch's other users are covered by the d8/d9 goldens."""
    _, _, words, most = _shape(HEAVY)
    assert words == 178711 and most <= 8
    _check(engine, HEAVY)


def test_state_across_runs_two_contexts():
    """16 runs of the second-group root on each of two contexts, from two
    threads at once: a call of 13 runs (the 8-run batch graph once and the
    one-run graph five times), then one of 3.  Every record is the oracle's and
    none has the overflow bit: a block's sums and gp_total carry nothing from
    one run, or from the other context, into the next."""
    want_tot, want_div = _oracle(BIG_W)
    p = dchess.pos_from_fen(BIG_W)
    engs = [dchess.Engine(0), dchess.Engine(0)]
    errs = []

    def work(e, buf, runs):
        try:
            e.perft_repeat_device(p, 7, 3, 0, 1, runs, buf)
            e.synchronize()
        except Exception as x:  # noqa: BLE001
            errs.append(x)

    bufs = []
    try:
        _, _, rm = engs[0].perft(p, 7)
        want = np.array([want_div[int(m)] for m in rm], np.uint64)
        for runs in (13, 3):
            bufs = [e.alloc(runs * W * 8) for e in engs]
            th = [threading.Thread(target=work, args=(e, b, runs)) for e, b in zip(engs, bufs)]
            for t in th:
                t.start()
            for t in th:
                t.join()
            assert not errs, errs
            for e, buf in zip(engs, bufs):
                res = buf.download(np.uint64, runs * W).reshape(runs, W)
                assert (res[:, 256] == len(rm)).all()  # n_root, no overflow bit
                assert (res[:, 257] == want_tot).all()
                assert (res[:, :len(rm)] == want).all() and not res[:, len(rm):256].any()
                assert _front(e) == 1
            for b in bufs:
                b.free()
            bufs = []
    finally:
        for b in bufs:
            b.free()
        for e in engs:
            e.close()
