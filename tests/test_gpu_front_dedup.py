"""GPU tests: the transposition dedup of the REF perft(6)/(7) front end
(k_front<.., DEDUP>, k_count3c<.., DEDUP>, k_front_fold).

A board reached by several move orders is handed to the final stage once; its
leaf count is folded into the divide entry of every root move it was reached
under.  Expected values come from the CPU oracle (oracle_lib) at run time or
from tests/golden."""
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
REF_D6 = json.load(open(os.path.join(GOLD, "ref_d6.json")))["positions"]
W = 258

# small roots with cross-root transpositions and childless grandparents
PAWNS = "8/p6p/8/P6K/8/8/8/8"
KNIGHT = "4k3/8/8/3n4/8/8/P7/4K3"
SMALL = {
    "pawns_w": (PAWNS + " w - - 0 1", {6: 1545, 7: 10968}),
    "pawns_b": (PAWNS + " b - - 0 1", {6: 924, 7: 1051}),
    "knight_w": (KNIGHT + " w - - 0 1", {7: 8146563}),
}


def _lib():
    L = dchess.lib()
    L.dc_test_perft_last_front.argtypes = [C.c_void_p]
    L.dc_test_front_dedup_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.dc_test_front_hash_mask.argtypes = [C.c_void_p, C.c_uint64]
    return L


def _front(e):
    return _lib().dc_test_perft_last_front(e.ctx)


def _stats(e):
    """(boards seen, owners, duplicates) of the context's last front run; zeros when it did not dedup."""
    out = (C.c_uint64 * 3)()
    assert _lib().dc_test_front_dedup_stats(e.ctx, out) == 0
    return tuple(int(x) for x in out)


_LEVELS = {}


def _levels(fen, plies):
    """Per ply: (nodes, distinct boards) of the REF tree below fen (oracle walk, computed once)."""
    key = (fen, plies)
    if key not in _LEVELS:
        cur = {O.Pos.from_fen(fen).cells.tobytes(): (O.Pos.from_fen(fen), 1)}
        out = [(1, 1)]
        for _ in range(plies):
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
            out.append((sum(m for _, m in cur.values()), len(cur)))
        _LEVELS[key] = out
    return _LEVELS[key]


_ORACLE = {}


def _oracle(fen, depth):
    key = (fen, depth)
    if key not in _ORACLE:
        tot, div, rm = O.fast_perft(O.Pos.from_fen(fen), depth)
        _ORACLE[key] = (tot, {int(m): int(v) for m, v in zip(rm, div)})
    return _ORACLE[key]


def _check(e, fen, depth, want_front=1):
    tot, div, rm = e.perft(dchess.pos_from_fen(fen), depth)
    want_tot, want_div = _oracle(fen, depth)
    assert tot == want_tot, (fen, depth)
    assert {int(m): int(v) for m, v in zip(rm, div)} == want_div, (fen, depth)
    assert _front(e) == want_front, (fen, depth)
    return tot


def _check_owners(e, fen, depth):
    """Where the run deduplicated, the owners are exactly the oracle's distinct grandparents."""
    seen, owners, dups = _stats(e)
    if depth == 7:
        assert seen > 0, "perft(7) unsharded runs the dedup"
    if seen:
        nodes, distinct = _levels(fen, depth - 3)[depth - 3]
        assert (seen, owners, dups) == (nodes, distinct, nodes - distinct), (fen, depth)


@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_roots(engine, name):
    fen, known = SMALL[name]
    for depth in (6, 7):
        for _ in range(2):  # the plain run, then the captured graph
            tot = _check(engine, fen, depth)
            if depth in known:
                assert tot == known[depth]
            _check_owners(engine, fen, depth)


def test_small_root_level_counts():
    """The oracle walk itself, against the counts the design note records."""
    lv = _levels(SMALL["pawns_w"][0], 4)
    assert lv[3] == (106, 55) and lv[4] == (181, 68)
    assert _levels(SMALL["pawns_b"][0], 4)[4] == (126, 54)
    assert _levels(SMALL["knight_w"][0], 4)[4] == (9269, 2146)


def test_startpos(engine):
    s = dchess.startpos()
    for depth, distinct in ((7, 72131), (6, None)):
        g = OG["perft_ref"]["startpos"][str(depth)]
        tot, div, rm = engine.perft(s, depth)
        assert tot == g["total"]
        assert {str(int(m)): int(v) for m, v in zip(rm, div)} == g["divide"]
        assert _front(engine) == 1
        seen, owners, dups = _stats(engine)
        if depth == 7:
            assert (seen, owners, dups) == (197742, 72131, 197742 - 72131)
        elif seen:
            start = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w - - 0 1"
            assert (seen, owners) == _levels(start, 3)[3] == (8902, 5362)


@pytest.mark.parametrize("name", sorted(SMALL) + ["mid0"])
def test_shards_sum(engine, name):
    """Depth 7 as 8 strided ply-3 shards: the summed divide is the unsharded one."""
    if name == "mid0":
        e = REF_D6[name]
        p = dchess.pos_from_cells(np.array(e["cells"], np.int8), e["stm"])
    else:
        p = dchess.pos_from_fen(SMALL[name][0])
    tot, div, rm = engine.perft(p, 7)
    if name != "mid0":  # (mid0's ply 4 is past the front end's 2^20 boards: unsharded it takes the chain)
        assert _front(engine) == 1
        want_tot, want_div = _oracle(SMALL[name][0], 7)
        assert tot == want_tot and {int(m): int(v) for m, v in zip(rm, div)} == want_div
    acc, t = np.zeros_like(div), 0
    for k in range(8):
        st, sd, srm = engine.perft_shard(p, 7, 3, k, 8)
        assert _front(engine) == 1
        assert (srm == rm).all()
        acc += sd
        t += st
    assert t == tot and (acc == div).all()


def test_state_hygiene_sequence():
    """One context: a declined position (the legacy chain), then front runs of
    other positions -- each correct and on the expected path."""
    e = dchess.Engine(0)
    try:
        for name, want in (("pos6", 0), ("mid4", 1)):
            r = REF_D6[name]
            p = dchess.pos_from_cells(np.array(r["cells"], np.int8), r["stm"])
            tot, div, rm = e.perft(p, 6)
            assert tot == r["total"]
            assert {str(int(m)): int(v) for m, v in zip(rm, div)} == r["divide"]
            assert _front(e) == want, name
        for name in sorted(SMALL):
            for depth in (6, 7):
                _check(e, SMALL[name][0], depth)
                _check_owners(e, SMALL[name][0], depth)
        g = OG["perft_ref"]["startpos"]["7"]
        tot, div, rm = e.perft(dchess.startpos(), 7)
        assert tot == g["total"] and _front(e) == 1
        assert {str(int(m)): int(v) for m, v in zip(rm, div)} == g["divide"]
        assert _stats(e)[1] == 72131
    finally:
        e.close()


def test_repeat_device_two_contexts():
    """19 runs of startpos perft(7) (two 8-run batch graphs and three single
    runs) on two contexts from two threads at once: every record is the golden,
    none has the overflow bit."""
    g = OG["perft_ref"]["startpos"]["7"]
    s = dchess.startpos()
    runs = 19
    engs = [dchess.Engine(0), dchess.Engine(0)]
    bufs = [e.alloc(runs * W * 8) for e in engs]
    errs = []

    def work(e, buf):
        try:
            e.perft_repeat_device(s, 7, 3, 0, 1, runs, buf)
            e.synchronize()
        except Exception as x:  # noqa: BLE001
            errs.append(x)

    try:
        _, _, rm = engs[0].perft(s, 7)
        want = np.array([g["divide"][str(int(m))] for m in rm], np.uint64)
        th = [threading.Thread(target=work, args=(e, b)) for e, b in zip(engs, bufs)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs
        for e, buf in zip(engs, bufs):
            res = buf.download(np.uint64, runs * W).reshape(runs, W)
            assert (res[:, 256] == len(rm)).all()  # n_root, no overflow bit
            assert (res[:, 257] == g["total"]).all()
            assert (res[:, :len(rm)] == want).all() and not res[:, len(rm):256].any()
            assert _front(e) == 1
    finally:
        for b in bufs:
            b.free()
        for e in engs:
            e.close()


def test_forced_collisions_decline():
    """With the hash cut to 8 bits nearly every match is a false one: each is
    caught by the board compare and the run declined (the legacy chain gives the
    result); no total is ever wrong.  The mask lives in the device-side
    descriptor, so captured graphs stay valid across a change of it: repeat
    graphs captured on the front path and replayed under the narrow mask decline
    inside the graph, and every record carries the overflow bit.  With the mask
    restored the front path is back on the same context."""
    L = _lib()
    e = dchess.Engine(0)
    s = dchess.startpos()
    FULL = 0xFFFFFFFFFFFFFFFF
    try:
        assert L.dc_test_front_hash_mask(e.ctx, 0xFF) == 0
        kfen = SMALL["knight_w"][0]
        kpos = dchess.pos_from_fen(kfen)
        want_tot, _ = _oracle(kfen, 7)
        for _ in range(2):  # (the second call declines again, then replays the chain's captured graph)
            _check(e, kfen, 7, want_front=0)
        g6 = OG["perft_ref"]["startpos"]["6"]
        tot, div, rm = e.perft(s, 6)
        assert tot == g6["total"]
        assert {str(int(m)): int(v) for m, v in zip(rm, div)} == g6["divide"]
        seen6 = _stats(e)[0]
        # (perft(6) declines only where it deduplicates: not in the product build)
        assert _front(e) == (0 if seen6 else 1)
        # repeat-device: capture the one-run and the 8-run graph on the front path (full mask) ...
        assert L.dc_test_front_hash_mask(e.ctx, FULL) == 0
        runs = 9
        buf = e.alloc(runs * W * 8)
        try:
            e.perft_repeat_device(kpos, 7, 3, 0, 1, runs, buf)
            e.synchronize()
            res = buf.download(np.uint64, runs * W).reshape(runs, W)
            assert _front(e) == 1
            assert not (res[:, 256] >> np.uint64(32)).any() and (res[:, 257] == want_tot).all()
            # ... and replay them under the narrow mask: the decline happens inside the graphs
            assert L.dc_test_front_hash_mask(e.ctx, 0xFF) == 0
            e.perft_repeat_device(kpos, 7, 3, 0, 1, runs, buf)
            e.synchronize()
            res = buf.download(np.uint64, runs * W).reshape(runs, W)
            assert ((res[:, 256] >> np.uint64(32)) == 1).all(), res[:, 256:]
            assert _front(e) == 1  # (the replays do not pass through the host's path choice)
            assert _stats(e)[0] > 0  # the deduplicating front end ran
            # the table was freed by each declined run: the same graphs, full mask again
            assert L.dc_test_front_hash_mask(e.ctx, FULL) == 0
            e.perft_repeat_device(kpos, 7, 3, 0, 1, runs, buf)
            e.synchronize()
            res = buf.download(np.uint64, runs * W).reshape(runs, W)
            assert not (res[:, 256] >> np.uint64(32)).any() and (res[:, 257] == want_tot).all()
        finally:
            buf.free()
        g7 = OG["perft_ref"]["startpos"]["7"]
        tot, div, rm = e.perft(s, 7)
        assert tot == g7["total"] and _front(e) == 1
        assert {str(int(m)): int(v) for m, v in zip(rm, div)} == g7["divide"]
        assert _stats(e)[1] == 72131
    finally:
        e.close()
