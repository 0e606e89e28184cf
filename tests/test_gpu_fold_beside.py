"""GPU tests: the perft(7) dedup fold and the result copy in the form that fits
beside the other context's kernels (k_front_fold at 32 registers and 2 KB of
LDS, one record per lane, the counts from the flags; k_copy_result as one wave;
DESIGN.md section 3.9).  Expected values come from the CPU oracle (oracle_lib)
at run time or from tests/golden.

The small roots are those of tests/test_gpu_front_dedup.py.  What they put
into one wave of 64 records is asserted from the oracle walk
(test_small_roots_mix_tags_in_a_wave).  Ply-4 nodes per root move: pawns_w 5,
48, 30, 46, 44, 8 (every one below 64: every wave holds several root tags);
pawns_b 58 and 68 (the first below 64: the wave that holds it holds the other
tag too); knight_w 996 to 1,652 under 7 root moves, none a multiple of 64 (the
tag boundaries fall inside waves).  Both pawn roots have childless ply-4
boards."""
import ctypes as C
import json
import os
import threading
import time

import numpy as np
import pytest

import dchess
import oracle_lib as O

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
OG = json.load(open(os.path.join(GOLD, "oracle_golden.json")))
W = 258

PAWNS = "8/p6p/8/P6K/8/8/8/8"
KNIGHT = "4k3/8/8/3n4/8/8/P7/4K3"
SMALL = {
    "pawns_w": PAWNS + " w - - 0 1",
    "pawns_b": PAWNS + " b - - 0 1",
    "knight_w": KNIGHT + " w - - 0 1",
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
    out = (C.c_uint64 * 3)()
    assert _lib().dc_test_front_dedup_stats(e.ctx, out) == 0
    return tuple(int(x) for x in out)


_WALK = {}


def _walk(fen):
    """Oracle walk to ply 4 (computed once per root): per root move the ply-4
    nodes and how many of them have no move, and the distinct ply-4 boards."""
    if fen not in _WALK:
        root = O.Pos.from_fen(fen)
        per_root, distinct = [], set()
        for m in O.fast_gen_moves(root):
            cur = [O.fast_make(root, int(m))]
            for _ in range(3):
                cur = [O.fast_make(p, int(x)) for p in cur for x in O.fast_gen_moves(p)]
            childless = sum(1 for p in cur if len(O.fast_gen_moves(p)) == 0)
            per_root.append((len(cur), childless))
            distinct.update(p.cells.tobytes() for p in cur)
        _WALK[fen] = (per_root, len(distinct))
    return _WALK[fen]


_ORACLE = {}


def _oracle(fen):
    if fen not in _ORACLE:
        tot, div, rm = O.fast_perft(O.Pos.from_fen(fen), 7)
        _ORACLE[fen] = (int(tot), {int(m): int(v) for m, v in zip(rm, div)})
    return _ORACLE[fen]


def test_small_roots_mix_tags_in_a_wave():
    per_root, _ = _walk(SMALL["pawns_w"])
    assert len(per_root) > 1 and all(n < 64 for n, _ in per_root), per_root
    assert sum(c for _, c in per_root) > 0, per_root  # childless boards among them
    per_root, _ = _walk(SMALL["pawns_b"])
    assert len(per_root) > 1 and min(n for n, _ in per_root) < 64, per_root
    assert sum(c for _, c in per_root) > 0, per_root
    per_root, _ = _walk(SMALL["knight_w"])
    assert len(per_root) > 1 and all(n % 64 for n, _ in per_root), per_root


@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_roots(engine, name):
    fen = SMALL[name]
    want_tot, want_div = _oracle(fen)
    per_root, distinct = _walk(fen)
    nodes = sum(n for n, _ in per_root)
    for _ in range(2):  # the plain run, then the captured graph
        tot, div, rm = engine.perft(dchess.pos_from_fen(fen), 7)
        assert tot == want_tot, name
        assert {int(m): int(v) for m, v in zip(rm, div)} == want_div, name
        assert _front(engine) == 1
        assert _stats(engine) == (nodes, distinct, nodes - distinct), name


def test_startpos(engine):
    """All 20 divide entries (1.2e8 to 2.0e8 each, sums of up to 64 totals of
    ~1e4 to 1e5 per wave) and a total of 3,282,734,510: past 2^31, the largest
    sums the shipped depth reaches (none passes 2^32)."""
    g = OG["perft_ref"]["startpos"]["7"]
    tot, div, rm = engine.perft(dchess.startpos(), 7)
    assert len(rm) == 20 and tot == g["total"] > 1 << 31
    assert {str(int(m)): int(v) for m, v in zip(rm, div)} == g["divide"]
    assert _front(engine) == 1
    assert _stats(engine) == (197742, 72131, 197742 - 72131)


def test_forced_collisions():
    """The hash cut to 8 bits: a plain perft still returns the oracle's count
    (through the decline path), and a repeat-device graph captured under the
    full mask and replayed under the narrow one carries the overflow bit."""
    L = _lib()
    FULL = 0xFFFFFFFFFFFFFFFF
    fen = SMALL["knight_w"]
    pos = dchess.pos_from_fen(fen)
    want_tot, want_div = _oracle(fen)
    e = dchess.Engine(0)
    try:
        assert L.dc_test_front_hash_mask(e.ctx, 0xFF) == 0
        tot, div, rm = e.perft(pos, 7)
        assert tot == want_tot and {int(m): int(v) for m, v in zip(rm, div)} == want_div
        assert _front(e) == 0
        assert L.dc_test_front_hash_mask(e.ctx, FULL) == 0
        runs = 3
        buf = e.alloc(runs * W * 8)
        try:
            e.perft_repeat_device(pos, 7, 3, 0, 1, runs, buf)
            e.synchronize()
            res = buf.download(np.uint64, runs * W).reshape(runs, W)
            assert _front(e) == 1
            assert not (res[:, 256] >> np.uint64(32)).any() and (res[:, 257] == want_tot).all()
            assert L.dc_test_front_hash_mask(e.ctx, 0xFF) == 0
            e.perft_repeat_device(pos, 7, 3, 0, 1, runs, buf)
            e.synchronize()
            res = buf.download(np.uint64, runs * W).reshape(runs, W)
            assert ((res[:, 256] >> np.uint64(32)) == 1).all(), res[:, 256:]
            # every slot was freed by the declined runs: the same graph, full mask again
            assert L.dc_test_front_hash_mask(e.ctx, FULL) == 0
            e.perft_repeat_device(pos, 7, 3, 0, 1, runs, buf)
            e.synchronize()
            res = buf.download(np.uint64, runs * W).reshape(runs, W)
            assert not (res[:, 256] >> np.uint64(32)).any() and (res[:, 257] == want_tot).all()
        finally:
            buf.free()
    finally:
        e.close()


def test_two_contexts_at_once():
    """24 repeat-device runs of startpos perft(7) on each of two contexts, from
    two threads: every record is the golden.  The device work is ~10 ms; the
    bound of 8 s on the whole test leaves room for two contexts and their graph
    captures and still ends a run in which a fold waits for the other context."""
    t_end = time.monotonic() + 8.0
    g = OG["perft_ref"]["startpos"]["7"]
    s = dchess.startpos()
    runs = 24
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
        th = [threading.Thread(target=work, args=(e, b), daemon=True) for e, b in zip(engs, bufs)]
        for t in th:
            t.start()
        for t in th:
            t.join(max(0.0, t_end - time.monotonic()))
        assert not any(t.is_alive() for t in th), "two contexts did not finish within the bound"
        assert not errs, errs
        for e, buf in zip(engs, bufs):
            res = buf.download(np.uint64, runs * W).reshape(runs, W)
            assert (res[:, 256] == len(rm)).all()  # n_root, no overflow bit
            assert (res[:, 257] == g["total"]).all()
            assert (res[:, :len(rm)] == want).all() and not res[:, len(rm):256].any()
        assert time.monotonic() < t_end
    finally:
        for b in bufs:
            b.free()
        for e in engs:
            e.close()
