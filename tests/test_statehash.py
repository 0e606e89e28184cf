"""State hash: keccak256(serde_json(GameState)),
core/src/consensus/hotstuff.rs:153-166.

CPU tests: the oracle (oracle/statehash.py) pinned against hashlib's SHA3-256
(same Keccak-f[1600]) and keccak256("") (the padding); the host product
(dc_keccak256, dchess.game_state_json) against the oracle.
GPU tests (marked): dc_state_hash over replay batches against the oracle's
move-by-move replay (refcpu verdicts, chess.rs history notation, JSON, keccak).
The reference holds no test or fixture of this hash: parity of the JSON layout
rests on prost/serde_json semantics restated in oracle/statehash.py (unpinned by
the reference)."""
import hashlib
import os
import sys

import numpy as np
import pytest

import dchess

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import statehash as S  # noqa: E402


# ------------------------------------------------------------------- CPU
def test_oracle_keccak_pinned():
    assert S.keccak256(b"").hex() == "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"
    rng = np.random.default_rng(1)
    for n in (0, 1, 135, 136, 137, 271, 272, 1000, 3000):
        d = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert S.sha3_256(d) == hashlib.sha3_256(d).digest(), n


def test_host_keccak_matches_oracle():
    rng = np.random.default_rng(2)
    for n in (0, 1, 7, 8, 135, 136, 137, 2500, 2999):
        d = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert dchess.keccak256(d) == S.keccak256(d), n


def test_host_keccak_every_length_to_300():
    """Every fill of the 136-byte rate, twice over: the 0x01 .. 0x80 padding
    at each position, 0x81 in one byte at 135 and 271, the extra all-padding
    block at 0, 136 and 272."""
    d = np.random.default_rng(4).integers(0, 256, 300, dtype=np.uint8).tobytes()
    for n in range(301):
        assert dchess.keccak256(d[:n]) == S.keccak256(d[:n]), n


# Unicode White_Space (Rust's char::is_whitespace, chess.rs:169-175) ...
WHITE_SPACE = ([0x20, 0x85, 0xA0, 0x1680, 0x2028, 0x2029, 0x202F, 0x205F, 0x3000]
               + list(range(0x09, 0x0E)) + list(range(0x2000, 0x200B)))
# ... and what is not: Python's str.split() splits at U+001C-U+001F, U+200B is
# a format character, U+180E left White_Space in Unicode 6.3
NOT_WHITE_SPACE = [0x1C, 0x1D, 0x1E, 0x1F, 0x200B, 0x180E]


@pytest.mark.parametrize("cp", WHITE_SPACE + NOT_WHITE_SPACE, ids=lambda cp: "U+%04X" % cp)
def test_history_token_count_is_rusts_white_space(cp):
    """update_history numbers a move 1 + split_whitespace().count(): the host
    (dc_history_append, the count dc_state_hash hands its kernel) and the
    oracle agree on "a" + ch + "b" + one move, for every White_Space
    character and for the near misses."""
    start = "a" + chr(cp) + "b"
    mv, info = np.array([12 | 28 << 6], np.uint16), np.array([0], np.uint8)  # e2e4: a pawn, no capture
    want = start + (" 3. e4" if cp in WHITE_SPACE else " 2. e4")
    assert S.append_history(start, "e4") == want
    assert dchess.history_append(start, mv, info) == want


NAMES = ["Alice", "Bob", 'q"uo\\te', "tab\tnew\nline\x01\x1f", "Ümlaut ♞ 名前", ""]


def _random_board(rng, n_pieces):
    cells = np.full(64, -1, np.int8)
    sq = rng.choice(64, n_pieces, replace=False)
    cells[sq] = rng.integers(0, 2, n_pieces) * 8 + rng.integers(0, 6, n_pieces)
    board = [[None] * 8 for _ in range(8)]
    for s in range(64):
        if cells[s] >= 0:
            board[s // 8][s % 8] = dchess.Piece(cells[s] >> 3, S.KIND[cells[s] & 7])
    return cells, board


def test_game_state_json_matches_oracle():
    rng = np.random.default_rng(3)
    for i in range(20):
        cells, board = _random_board(rng, int(rng.integers(0, 33)))
        w, b = NAMES[i % len(NAMES)], NAMES[(i + 2) % len(NAMES)]
        hist = None if i == 7 else ("" if i % 3 == 0 else "1. e4 3. Nf6 5. exd5")
        turn = i & 1
        assert dchess.game_state_json(turn, w, b, hist, board) == S.game_state_json(turn, w, b, hist, cells)


def test_unknown_kind_string_serialised():
    board = [[None] * 8 for _ in range(8)]
    board[3][4] = dchess.Piece(1, "Dragon")
    cells = np.full(64, -1, np.int8)
    cells[28] = 8 + 6
    assert dchess.game_state_json(0, "a", "b", "", board) == S.game_state_json(0, "a", "b", "", cells,
                                                                               kinds={28: "Dragon"})


# ------------------------------------------------------------------- GPU
def _oracle_walk(start, history, col):
    """One game move by move: refcpu verdicts (chess.rs:82-125), apply
    (chess.rs:72-77), update_history (chess.rs:127-184).  Yields (n, stm,
    history, cells, event) for n = 0 .. len(col): the state after the first n
    plies (cells is the walk's own array: copy it to keep it) and what ply
    n - 1 did: None for n = 0 and for a rejected ply, else (kind, capture)."""
    import oracle_lib as O
    cells, stm, hist = start.cells.copy(), start.stm, history
    yield 0, stm, hist, cells, None
    for p in range(len(col)):
        m, ev = int(col[p]), None
        f, t = m & 63, (m >> 6) & 63
        if (m != O.SENTINEL and not m & 0x8000
                and O.ref_validate(cells, stm, f >> 3, f & 7, t >> 3, t & 7) == O.OK):
            ev = (int(cells[f]) & 7, bool(cells[t] >= 0))
            hist = S.append_history(hist, S.notation(S.KIND[ev[0]], ev[1], f, t))
            cells[t], cells[f] = cells[f], -1
            stm ^= 1
        yield p + 1, stm, hist, cells, ev


def _oracle_hash(stm, names, hist, cells):
    """serde_json, keccak256 of one final state, as a uint8[32] row."""
    return np.frombuffer(S.keccak256(S.game_state_json(stm, names[0], names[1], hist, cells).encode()), np.uint8)


def _oracle_hashes(start, history, names, mv):
    """Every game walked move by move (_oracle_walk), then serde_json, keccak256."""
    n_plies, n_games = mv.shape
    out = np.zeros((n_games, 32), np.uint8)
    for g in range(n_games):
        for _, stm, hist, cells, _ in _oracle_walk(start, history, mv[:, g]):
            pass
        out[g] = _oracle_hash(stm, names[g], hist, cells)
    return out


def _games(seed, n_games, n_plies, start):
    import oracle_lib as O
    rng = np.random.default_rng(seed)
    mv = np.full((n_plies, n_games), O.SENTINEL, np.uint16)
    for g in range(n_games):
        p = start.copy()
        for ply in range(n_plies if rng.random() < 0.85 else int(rng.integers(0, n_plies))):
            legal = O.fast_gen_moves(p)
            r = rng.random()
            m = int(rng.choice(legal)) if (r < 0.75 and len(legal)) else (
                int(rng.integers(0, 4096)) if r < 0.97 else 0x8000 | int(rng.integers(0, 0x7FFF)))
            mv[ply, g] = m
            if not m & 0x8000 and O.fast_validate(p, m) == O.OK:
                p = O.fast_make(p, m)
    return mv


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["startpos", "midgame_black_history"])
def test_state_hash_batch_vs_oracle(engine, case):
    import oracle_lib as O
    if case == "startpos":
        start, history, dstart = O.Pos(), "", None
    else:
        mv0 = O.fast_gen_games(77, 0, 1, 30, noise_per_256=0)
        start = O.Pos()
        for p in range(30):
            start = O.fast_make(start, int(mv0[p, 0]))
        start.castle, start.ep = 0, -1
        start.stm = 1
        history = "1. e4 3. e5\tnote  5. Nf3"
        dstart = dchess.pos_from_cells(start.cells, start.stm)
    n_games = 70 if case == "startpos" else 33
    mv = _games(11, n_games, 41, start)
    names = [(NAMES[g % len(NAMES)] + str(g), NAMES[(g * 5 + 1) % len(NAMES)]) for g in range(n_games)]
    got = engine.state_hash(mv, names, start=dstart, history=history)
    want = _oracle_hashes(start, history, names, mv)
    assert (got == want).all()


@pytest.mark.gpu
def test_state_hash_without_replay_prepass(engine):
    """when the replay pre-pass's buffers cannot be had (forced here
    through the test hook dc_test_hash_prepass_max = 0), the hash kernel's own
    validation path runs instead of the call failing, with the same hashes."""
    import ctypes as C
    import oracle_lib as O
    L = dchess.lib()
    L.dc_test_hash_prepass_max.argtypes = [C.c_void_p, C.c_uint64]
    mv = _games(12, 45, 33, O.Pos())
    names = [(NAMES[g % len(NAMES)], NAMES[(g * 3 + 2) % len(NAMES)] + str(g)) for g in range(45)]
    with_pre = engine.state_hash(mv, names)
    try:
        assert L.dc_test_hash_prepass_max(engine.ctx, 0) == 0
        without = engine.state_hash(mv, names)
    finally:
        L.dc_test_hash_prepass_max(engine.ctx, 2**64 - 1)
    assert (with_pre == without).all()
    assert (without == _oracle_hashes(O.Pos(), "", names, mv)).all()


@pytest.mark.gpu
def test_state_hash_move_numbers_by_division(engine):
    """The hash kernel keeps the history's move numbers as 32-bit BCD when
    every number of the batch stays below 10^7, else it divides by 10; the
    test hook dc_test_hash_bcd_max lowers that bound so the division path runs
    (a start history of several tokens, numbers into three digits), with the
    same hashes as the BCD path and the oracle."""
    import ctypes as C
    import oracle_lib as O
    L = dchess.lib()
    L.dc_test_hash_bcd_max.argtypes = [C.c_void_p, C.c_uint32]
    mv = _games(14, 40, 61, O.Pos())
    names = [(NAMES[g % len(NAMES)], "b" + str(g)) for g in range(40)]
    history = "1. e4 e5 2. Nf3 " + " ".join(str(k) for k in range(40))
    bcd = engine.state_hash(mv, names, history=history)
    try:
        assert L.dc_test_hash_bcd_max(engine.ctx, 1) == 0
        div = engine.state_hash(mv, names, history=history)
    finally:
        L.dc_test_hash_bcd_max(engine.ctx, 10**7)
    assert (bcd == div).all()
    assert (div == _oracle_hashes(O.Pos(), history, names, mv)).all()


@pytest.mark.gpu
def test_state_hash_matches_gamestate_mirror(engine):
    """One game through the Python GameState mirror (dc_apply_batch per move,
    host JSON + dc_keccak256) and through the batched kernel."""
    import oracle_lib as O
    gs = dchess.GameState("Alice", "Bob", engine)
    mv = O.fast_gen_games(5, 0, 1, 24, noise_per_256=0)
    for p in range(24):
        m = int(mv[p, 0])
        f, t = m & 63, (m >> 6) & 63
        gs.apply_move(dchess.Position(f >> 3, f & 7), dchess.Position(t >> 3, t & 7))
    got = engine.state_hash(mv, [("Alice", "Bob")])
    assert "0x" + bytes(got[0]).hex() == gs.state_hash()


@pytest.mark.gpu
def test_state_hash_edge_cases(engine):
    # no plies: the start state's hash; unknown-kind start rejected
    got = engine.state_hash(np.zeros((0, 3), np.uint16), [("w", "b")] * 3)
    import oracle_lib as O
    want = S.keccak256(S.game_state_json(0, "w", "b", "", O.startpos_cells()).encode())
    assert all(bytes(r) == want for r in got)
    cells = np.full(64, -1, np.int8)
    cells[0], cells[63] = 5, 8 + 6  # white king, black unknown kind
    with pytest.raises(dchess.DChessError):
        engine.state_hash(np.zeros((2, 1), np.uint16), [("w", "b")], start=dchess.pos_from_cells(cells, 0))


@pytest.mark.gpu
def test_state_hash_device_resident_names(engine):
    """dc_state_hash_device with moves, raw names and hashes resident on the
    device: the names are escaped on the GPU (k_escape_len / scan /
    k_escape_write, serde_json's table).  Every byte 0x00-0x1f, '"', '\\\\',
    0x7f and multi-byte UTF-8 appear in some name; checked against the oracle
    and against the host-buffer entry point."""
    import oracle_lib as O
    start = O.Pos()
    n_games, n_plies = 67, 23
    mv = _games(29, n_games, n_plies, start)
    ctrl = "".join(chr(c) for c in range(0x20))
    pool = NAMES + [ctrl, 'x"\\\x7f\b\f\r', "♞" * 40, "a" * 300]
    names = [(pool[g % len(pool)], pool[(g * 3 + 2) % len(pool)] + str(g)) for g in range(n_games)]
    blob, off = dchess.pack_names(names)
    d_names, d_off = engine.names_device(blob, off)
    d_moves = engine.alloc(mv.nbytes)
    d_moves.upload(mv)
    d_h = engine.alloc(32 * n_games)
    history = "1. e4\x0c"
    engine.state_hash_device(d_moves, n_games, n_plies, d_names, d_off, d_h, history=history)
    got = d_h.download(np.uint8, 32 * n_games).reshape(n_games, 32)
    want = _oracle_hashes(start, history, names, mv)
    assert (got == want).all()
    assert (engine.state_hash(mv, names, history=history) == want).all()
    for b in (d_names, d_off, d_moves, d_h):
        b.free()


@pytest.mark.gpu
def test_state_hash_plain_names_read_in_place(engine):
    """Names with no byte serde_json escapes (ASCII letters, digits, 0x7f,
    multi-byte UTF-8, empty names) take the fast path: k_names_plain finds
    nothing to escape and the hash kernel reads the raw names and offsets in
    place.  Checked against the oracle, with a start history that is escaped
    (its own path), and against a batch where one name needs an escape."""
    import oracle_lib as O
    start = O.Pos()
    n_games, n_plies = 70, 19
    mv = _games(31, n_games, n_plies, start)
    pool = ["Alice", "Bob", "Ümlaut ♞ 名前", "", "a" * 300, "x\x7fy", "white123456"]
    names = [(pool[g % len(pool)], pool[(g * 3 + 2) % len(pool)] + str(g)) for g in range(n_games)]
    history = "1. e4 e5\t"
    for nm in (names, names[:-1] + [("tab\there", "q\"")]):
        blob, off = dchess.pack_names(nm)
        d_names, d_off = engine.names_device(blob, off)
        d_moves = engine.alloc(mv.nbytes)
        d_moves.upload(mv)
        d_h = engine.alloc(32 * n_games)
        engine.state_hash_device(d_moves, n_games, n_plies, d_names, d_off, d_h, history=history)
        got = d_h.download(np.uint8, 32 * n_games).reshape(n_games, 32)
        assert (got == _oracle_hashes(start, history, nm, mv)).all()
        for b in (d_names, d_off, d_moves, d_h):
            b.free()


@pytest.mark.gpu
def test_state_hash_rejects_decreasing_offsets(engine):
    blob, off = dchess.pack_names([("ab", "cd")])
    off = off.copy()
    off[1], off[2] = 3, 1
    mv = np.zeros((1, 1), np.uint16)
    with pytest.raises(dchess.DChessError):
        _raw_state_hash(engine, mv, blob, off)


def _raw_state_hash(engine, mv, blob, off):
    import ctypes as C
    out = np.zeros((mv.shape[1], 32), np.uint8)
    st = dchess.lib().dc_state_hash(engine.ctx, None, b"", blob, C.c_void_p(off.ctypes.data),
                                     C.c_void_p(mv.ctypes.data), mv.shape[1], mv.shape[0],
                                     C.c_void_p(out.ctypes.data))
    dchess._check(st, "dc_state_hash")
