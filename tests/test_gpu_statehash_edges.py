"""dc_state_hash where k_state_hash_ref branches: every message length modulo
Keccak's 136-byte rate, batches past one block of 256 lanes, games past the
128 plies whose verdicts pass 1 keeps, the clamps of the pre-pass loops at
short games, move numbers that gain a digit, and the switch between BCD and
division.  Every hash is compared with oracle/statehash.py, walked move by
move with refcpu verdicts (test_statehash._oracle_walk); the seven-digit move
numbers, whose 2 MB history the Python Keccak cannot hash, are checked on the
device by the hook dc_test_hash_digits over the helpers the kernel calls."""
import ctypes as C
from contextlib import contextmanager

import numpy as np
import pytest

import dchess
import oracle_lib as O
from test_statehash import NAMES, S, _games, _oracle_hash, _oracle_hashes, _oracle_walk

pytestmark = pytest.mark.gpu

RATE = 136


# ------------------------------------------------------------------ helpers
@contextmanager
def _no_prepass(engine):
    """The hash kernel validates on its own (info == nullptr)."""
    L = dchess.lib()
    L.dc_test_hash_prepass_max.argtypes = [C.c_void_p, C.c_uint64]
    try:
        assert L.dc_test_hash_prepass_max(engine.ctx, 0) == 0
        yield
    finally:
        L.dc_test_hash_prepass_max(engine.ctx, 2**64 - 1)


@contextmanager
def _bcd_max(engine, bound):
    """Move numbers are BCD only while all of a batch's stay below bound."""
    L = dchess.lib()
    L.dc_test_hash_bcd_max.argtypes = [C.c_void_p, C.c_uint32]
    try:
        assert L.dc_test_hash_bcd_max(engine.ctx, bound) == 0
        yield
    finally:
        L.dc_test_hash_bcd_max(engine.ctx, 10**7)


def _hash_device(engine, mv, names, history):
    """dc_state_hash_device: moves, raw names and hashes resident on the device."""
    n_plies, n_games = mv.shape
    blob, off = dchess.pack_names(names)
    d_names, d_off = engine.names_device(blob, off)
    d_moves = engine.alloc(max(mv.nbytes, 2))
    d_h = engine.alloc(32 * n_games)
    try:
        if mv.nbytes:
            d_moves.upload(mv)
        engine.state_hash_device(d_moves, n_games, n_plies, d_names, d_off, d_h, history=history)
        return d_h.download(np.uint8, 32 * n_games).reshape(n_games, 32)
    finally:
        for b in (d_names, d_off, d_moves, d_h):
            b.free()


def _same(got, want):
    """All hashes equal; on failure the message names the games, not 32 x n bytes."""
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} of {len(want)} hashes differ, games {bad[:12].tolist()}"


# ------------------------------------- 2. every length modulo the rate, 280 lanes
N_RESIDUE = 280  # one block of 256 lanes and 24 lanes of a second
UNITS = {
    "plain": ("", "a"),        # read in place
    "escaped": ("\x1f", "a"),  # the batch goes through the device's escaping; \u001f straddles blocks
    "utf8": ("", "名"),        # three bytes a character: 3 g mod 136 takes every value
}
HIST_WS = "1. e4\t3. e5\u2003note"  # a tab (escaped as \t) and U+2003 (White_Space, three bytes): 5 tokens


@pytest.fixture(scope="module")
def base_games():
    """name -> (start history, move column, final (stm, history, cells), per-ply events)."""
    out = {}
    for name, history, col in (
            ("no_plies", "", np.zeros(0, np.uint16)),
            ("sixty_plies", HIST_WS, O.fast_gen_games(2024, 0, 1, 60, noise_per_256=24)[:, 0])):
        events = []
        for _, stm, hist, cells, ev in _oracle_walk(O.Pos(), history, col):
            events.append(ev)
        out[name] = (history, col, (stm, hist, cells.copy()), events[1:])
    ev = out["sixty_plies"][3]
    assert sum(e is not None and e[1] for e in ev) >= 3 and any(e is None for e in ev), "captures and rejected plies"
    return out


_residue_cache = {}


def _residue_batch(base_games, family, base):
    """(names, oracle JSON, oracle hashes) of the 280 games: computed once."""
    if (family, base) not in _residue_cache:
        head, unit = UNITS[family]
        stm, hist, cells = base_games[base][2]
        names = [(head + unit * g, "b") for g in range(N_RESIDUE)]
        js = [S.game_state_json(stm, w, b, hist, cells) for w, b in names]
        want = np.stack([np.frombuffer(S.keccak256(j.encode()), np.uint8) for j in js])
        _residue_cache[family, base] = (names, js, want)
    return _residue_cache[family, base]


@pytest.mark.parametrize("base", ["no_plies", "sixty_plies"])
@pytest.mark.parametrize("family", list(UNITS))
def test_every_length_modulo_the_rate(engine, base_games, family, base):
    """Game g's white name is g units long and all else is shared, so the 280
    streams step through every fill of the last block at least twice: the
    0x01 at each offset, 0x81 in byte 135, the all-padding block after a
    stream that ends on a boundary; and every piece after the name starts at
    every offset of a block.  Lanes 256-279 run in a second block beside 232
    inactive ones."""
    history, col, _, _ = base_games[base]
    names, js, want = _residue_batch(base_games, family, base)
    residues = {len(j.encode()) % RATE for j in js}
    assert residues == set(range(RATE)), sorted(set(range(RATE)) - residues)
    assert all(sum(len(j.encode()) % RATE == r for j in js) >= 2 for r in (0, 1, RATE - 1))
    mv = np.ascontiguousarray(np.repeat(col[:, None], N_RESIDUE, axis=1))
    _same(engine.state_hash(mv, names, history=history), want)
    _same(_hash_device(engine, mv, names, history), want)
    with _no_prepass(engine):
        _same(engine.state_hash(mv, names, history=history), want)


@pytest.mark.parametrize("base", ["no_plies", "sixty_plies"])
def test_host_mirror_at_the_same_lengths(base_games, base):
    """The host's own path to the same value (dc_history_append, the package's
    JSON, dc_keccak256), for every 14th game of the three families."""
    history, col, (stm, _, cells), events = base_games[base]
    info = np.array([0xFF if e is None else e[0] | 8 * e[1] for e in events], np.uint8)
    hist = dchess.history_append(history, col, info)
    board = [[None if cells[8 * x + y] < 0 else dchess.Piece(cells[8 * x + y] >> 3, S.KIND[cells[8 * x + y] & 7])
              for y in range(8)] for x in range(8)]
    for family in UNITS:
        names, _, want = _residue_batch(base_games, family, base)
        for g in range(0, N_RESIDUE, 14):
            js = dchess.game_state_json(stm, names[g][0], names[g][1], hist, board)
            assert dchess.keccak256(js.encode()) == bytes(want[g]), (family, g)


@pytest.fixture(scope="module")
def mixed_batch():
    """513 games of their own moves and names; a smaller batch is its first n."""
    n_games, history = 513, "1. e4\x0c"
    mv = _games(41, n_games, 9, O.Pos())
    pool = NAMES + ["x\x7fy", "♞" * 45, "a" * 136, "a" * 135]
    names = [(pool[g % len(pool)] + str(g), pool[(g * 7 + 3) % len(pool)]) for g in range(n_games)]
    return history, mv, names, _oracle_hashes(O.Pos(), history, names, mv)


@pytest.mark.parametrize("n_games", [1, 255, 256, 257, 513])
def test_batch_sizes_around_a_block_of_lanes(engine, mixed_batch, n_games):
    """One lane, a block less one, a full block, a block and one lane, two
    blocks and one lane (the move words' stride is the batch size)."""
    history, mv, names, want = mixed_batch
    sub = np.ascontiguousarray(mv[:, :n_games])
    _same(engine.state_hash(sub, names[:n_games], history=history), want[:n_games])
    _same(_hash_device(engine, sub, names[:n_games], history), want[:n_games])
    with _no_prepass(engine):
        _same(engine.state_hash(sub, names[:n_games], history=history), want[:n_games])


# ------------------------------------------------- 3. long and very short games
# around the pre-pass loops' batch of 16 and queue of 4, and around the 128
# plies whose verdicts the kernel keeps when there is no pre-pass
PREFIXES = [1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 127, 128, 129, 160, 200]


@pytest.fixture(scope="module")
def long_games():
    """48 games x 200 plies; the oracle walks each once and hashes it at every prefix."""
    n_games, n_plies = 48, 200
    mv = _games(53, n_games, n_plies, O.Pos())
    names = [(NAMES[g % len(NAMES)] + str(g), NAMES[(g * 5 + 1) % len(NAMES)]) for g in range(n_games)]
    want = {n: np.zeros((n_games, 32), np.uint8) for n in PREFIXES}
    late = {"accepted": 0, "rejected": 0, "captures": 0}
    for g in range(n_games):
        for n, stm, hist, cells, ev in _oracle_walk(O.Pos(), "", mv[:, g]):
            if n in want:
                want[n][g] = _oracle_hash(stm, names[g], hist, cells)
            if n > 128 and mv[n - 1, g] != O.SENTINEL:
                late["accepted" if ev else "rejected"] += 1
                late["captures"] += bool(ev and ev[1])
    # plies 128.. (validated again in pass 2 when there is no pre-pass) accept, reject and capture
    assert late["accepted"] >= 100 and late["rejected"] >= 100 and late["captures"] >= 10, late
    return mv, names, want


@pytest.mark.parametrize("n_plies", PREFIXES)
def test_prefixes_of_long_games(engine, long_games, n_plies):
    mv, names, want = long_games
    sub = np.ascontiguousarray(mv[:n_plies])
    _same(engine.state_hash(sub, names), want[n_plies])
    with _no_prepass(engine):
        _same(engine.state_hash(sub, names), want[n_plies])


# --------------------------------------------------------------- 4. move numbers
N_NUM_PLIES = 12


def _number_case(k, n_games):
    history = "a " * k
    mv = _games(61 + k % 7, n_games, N_NUM_PLIES, O.Pos())
    names = [("w%d" % g, "b") for g in range(n_games)]
    want, numbers = np.zeros((n_games, 32), np.uint8), set()
    for g in range(n_games):
        for _, stm, hist, cells, ev in _oracle_walk(O.Pos(), history, mv[:, g]):
            if ev:
                numbers.add(int(hist.rsplit(" ", 2)[1][:-1]))
        want[g] = _oracle_hash(stm, names[g], hist, cells)
    return history, mv, names, want, numbers


# a start history of k tokens numbers the moves k + 1, k + 3, ...: both parities below each power of ten
@pytest.mark.parametrize("k,n_games", [(90, 8), (91, 8), (990, 8), (991, 8), (9990, 8), (9991, 8), (99990, 3)])
def test_move_numbers_gain_a_digit(engine, k, n_games):
    """bcd_add2's carries through two to five nines, the digit count and the
    digit extraction at each new length, against the same numbers by
    division, both against the oracle."""
    history, mv, names, want, numbers = _number_case(k, n_games)
    top = 10 ** len(str(k))
    below, above = (top - 1, top + 1) if k % 2 == 0 else (top - 2, top)
    assert {below, above} <= numbers, sorted(numbers)
    _same(engine.state_hash(mv, names, history=history), want)  # BCD
    with _bcd_max(engine, 1):
        _same(engine.state_hash(mv, names, history=history), want)  # division
    with _no_prepass(engine):
        _same(engine.state_hash(mv, names, history=history), want)


def test_bcd_bound_on_both_sides(engine):
    """bcd_ok = hist_tokens + 2 n_plies + 1 < bound: the bound set to exactly
    that sum (division) and to one more (BCD)."""
    k = 990
    history, mv, names, want, _ = _number_case(k, 8)
    edge = k + 2 * N_NUM_PLIES + 1
    for bound in (edge, edge + 1):
        with _bcd_max(engine, bound):
            _same(engine.state_hash(mv, names, history=history), want)


def test_move_number_digits_to_ten_million(engine):
    """Every number the BCD path can meet: for each v in [1, 10^7) the digits
    bcd_emit writes are v's and equal div_emit's, and bcd_add2(bcd(v)) is
    bcd(v + 2) -- on the device, over the helpers k_state_hash_ref calls."""
    L = dchess.lib()
    L.dc_test_hash_digits.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    L.dc_test_hash_digits.restype = C.c_int
    out = np.full(2, 7, np.uint32)
    dchess._check(L.dc_test_hash_digits(engine.ctx, 1, 10**7 - 1, C.c_void_p(out.ctypes.data)), "dc_test_hash_digits")
    assert out.tolist() == [0, 0xFFFFFFFF]
    # the hook refuses what the kernel never meets: 0 and numbers of eight digits
    assert L.dc_test_hash_digits(engine.ctx, 0, 10, C.c_void_p(out.ctypes.data)) == dchess.EINVAL
    assert L.dc_test_hash_digits(engine.ctx, 1, 10**7, C.c_void_p(out.ctypes.data)) == dchess.EINVAL
