"""CPU tests of the notation entry points: dc_san_format, dc_pgn_movetext and
dc_pos_to_fen run on the host and are compared with the formatter of the SAN
model (tests/san_model.py, which never calls them); dc_replay_san* are exported
and reject a NULL context before any device is touched."""
import ctypes as C
import itertools
import json
import os
import re

import numpy as np
import pytest

import dchess
import oracle_lib as O
import outcome_model as M
import san_model as S
from test_outcome_model import PINNED
from test_san_model import LINES, MOVETEXT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dchess.h")
GOLDEN = os.path.join(ROOT, "tests", "golden")
DRAWS = (dchess.GO_STALEMATE, dchess.GO_DEAD, dchess.GO_FIVEFOLD, dchess.GO_SEVENTYFIVE)


def raw_format(move, san):
    buf = C.create_string_buffer(b"\x7f" * 8, 8)
    return dchess.lib().dc_san_format(move, san, buf), buf


def raw_movetext(moves, san, n, stride, fullmove, stm, result, cap):
    buf = C.create_string_buffer(max(cap, 1))
    n_out = C.c_size_t(12345)
    r = dchess.lib().dc_pgn_movetext(dchess._ptr(moves), dchess._ptr(san), n, stride, fullmove, stm, result,
                                     buf if cap else None, cap, C.byref(n_out))
    return r, n_out.value, buf.value.decode()


def test_library_exports_notation_symbols():
    L = dchess.lib()
    names = dchess.exported_symbols()
    for n in ("dc_replay_san", "dc_replay_san_device", "dc_san_format", "dc_pgn_movetext", "dc_pos_to_fen"):
        assert n in names, n
        assert hasattr(L, n), n


def test_san_constants_match_header():
    hdr = open(HEADER).read()
    vals = {m.group(1): int(m.group(2), 16) for m in re.finditer(r"#define\s+DC_SAN_(\w+)\s+0x([0-9A-Fa-f]+)u", hdr)}
    assert vals == {"CAPTURE": dchess.SAN_CAPTURE, "FILE": dchess.SAN_FILE, "RANK": dchess.SAN_RANK,
                    "CHECK": dchess.SAN_CHECK, "MATE": dchess.SAN_MATE}
    assert vals == {"CAPTURE": S.CAPTURE, "FILE": S.FILE, "RANK": S.RANK, "CHECK": S.CHECK, "MATE": S.MATE}
    assert dchess.SAN_NONE == S.NONE == 0xFF
    assert '"replay_san"' in hdr  # the kernel-name list


def test_san_format_every_flag_combination():
    """Every kind x capture x (none, file, rank, both) x (none, check, mate) on a
    plain move, against the model's formatter."""
    mv = M.mv("c3e4")  # no castle, no promotion rank
    seen = set()
    for kind, cap, dis, chk in itertools.product(range(6), (0, S.CAPTURE), (0, S.FILE, S.RANK, S.FILE | S.RANK),
                                                 (0, S.CHECK, S.CHECK | S.MATE)):
        byte = kind | cap | dis | chk
        got = dchess.san_format(mv, byte)
        assert got == S.san_text(mv, byte), byte
        assert len(got) <= 7
        seen.add(got)
    assert len(seen) == 5 * 2 * 4 * 3 + 2 * 3  # a pawn's token ignores the origin flags
    assert dchess.san_format(M.mv("h4e1"), M.Q | S.FILE | S.RANK | S.CAPTURE | S.CHECK | S.MATE) == "Qh4xe1#"
    # MATE without CHECK (never produced) still prints '#'
    assert dchess.san_format(mv, M.N | S.MATE) == "Ne4#"


def test_san_format_promotions_and_castles():
    for text, byte in (("e7e8q", M.P), ("e7e8n", M.P | S.CHECK), ("e7d8r", M.P | S.CAPTURE), ("b2a1b", M.P | S.CAPTURE),
                       ("a2a1q", M.P | S.CHECK | S.MATE), ("h7g8q", M.P | S.CAPTURE | S.CHECK | S.MATE),
                       ("e1g1", M.K), ("e1c1", M.K | S.CHECK), ("e8g8", M.K | S.CHECK | S.MATE), ("e8c8", M.K),
                       ("e1f1", M.K), ("e1e2", M.K | S.CAPTURE), ("e1g1", M.R), ("e4g4", M.K)):
        mv = M.mv(text)
        assert dchess.san_format(mv, byte) == S.san_text(mv, byte), text
    assert dchess.san_format(M.mv("h7g8q"), M.P | S.CAPTURE | S.CHECK | S.MATE) == "hxg8=Q#"
    assert dchess.san_format(M.mv("e8c8"), M.K) == "O-O-O"
    assert dchess.san_format(M.mv("e1g1"), M.K | S.CHECK) == "O-O+"
    assert dchess.san_format(M.mv("e1g1"), M.R) == "Rg1"  # a rook on e1, not a castle
    assert dchess.san_format(M.mv("e1g3"), M.K) == "Kg3"  # two files, another rank: no castle (and no legal move)


def test_san_format_einval():
    e2e4, e7e8 = M.mv("e2e4"), M.mv("e7e8")
    bad = [(e2e4, 0xFF), (e2e4, 6), (e2e4, 7), (e2e4, 6 | S.CAPTURE), (e2e4 | dchess.MOVE_OOR, M.P),
           (dchess.MOVE_NONE, M.P),
           (e2e4 | (1 << 12), M.N),      # a promotion by a piece
           (e2e4 | (4 << 12), M.K),
           (e2e4 | (5 << 12), M.P),      # promo above 4
           (e7e8 | (5 << 12), M.P), (e7e8 | (7 << 12), M.P),
           (e2e4 | (4 << 12), M.P),      # a promotion short of the last rank
           (e7e8, M.P),                  # a pawn on the last rank without one
           (M.mv("e2e1"), M.P)]
    for mv, byte in bad:
        r, buf = raw_format(mv, byte)
        assert r == dchess.EINVAL, (hex(mv), byte)
    assert dchess.lib().dc_san_format(e2e4, M.P, None) == dchess.EINVAL
    with pytest.raises(dchess.DChessError) as e:
        dchess.san_format(e2e4, 0xFF)
    assert e.value.status == dchess.EINVAL
    # the longest token fills out[8] exactly, NUL included
    r, buf = raw_format(M.mv("h4e1"), M.Q | S.FILE | S.RANK | S.CAPTURE | S.MATE)
    assert r == 0 and buf.raw == b"Qh4xe1#\0"


@pytest.mark.parametrize("fen,moves,want", LINES, ids=[str(i) for i in range(len(LINES))])
def test_pinned_lines_through_the_formatter(fen, moves, want):
    start = O.Pos.from_fen(fen) if fen else None
    mv = M.line(moves)
    r = S.annotate(mv, start)
    assert " ".join(dchess.san_format(m, b) for m, b in zip(mv, r["san"])) == want


@pytest.mark.parametrize("name,fen,halfmove,moves,want", PINNED, ids=[p[0] for p in PINNED])
def test_movetext_pinned_games(name, fen, halfmove, moves, want):
    """White-first and Black-first starts (fivefold_live_ep), skipped 0xFF plies
    (illegal_first_move, the plies after a game's end), the empty game."""
    start = O.Pos.from_fen(fen) if fen else None
    mv = M.line(moves)
    r = S.annotate(mv, start, halfmove)
    got = dchess.pgn_movetext(mv, r["san"], r["result"], 1, start.stm if start else 0)
    assert got == MOVETEXT[name]
    assert got == S.movetext(mv, r["san"], r["result"], 1, start.stm if start else 0)


def test_movetext_numbers_and_first_side():
    mv = np.array(M.line("e7e5 g1f3 b8c6 f1b5"), np.uint16)
    san = np.array([M.P, M.N, M.N, M.B], np.uint8)
    assert dchess.pgn_movetext(mv, san, dchess.GO_ONGOING, 1, 1) == "1... e5 2. Nf3 Nc6 3. Bb5 *"
    assert dchess.pgn_movetext(mv, san, dchess.GO_ONGOING, 41, 1) == "41... e5 42. Nf3 Nc6 43. Bb5 *"
    assert dchess.pgn_movetext(mv, san, dchess.GO_ONGOING, 41, 0) == "41. e5 Nf3 42. Nc6 Bb5 *"
    assert dchess.pgn_movetext(mv[:1], san[:1], dchess.GO_ONGOING, 9, 1) == "9... e5 *"
    # a skipped first ply: the first WRITTEN move is Black's
    san2 = san.copy()
    san2[0] = 0xFF
    assert dchess.pgn_movetext(mv, san2, dchess.GO_ONGOING, 3, 1) == "3... Nf3 4. Nc6 Bb5 *"
    assert dchess.pgn_movetext(mv, san2, dchess.GO_ONGOING, 3, 1) == S.movetext(mv, san2, M.ONGOING, 3, 1)
    # skipped plies in the middle do not pass the turn
    san3 = np.array([M.P, 0xFF, 0xFF, M.B], np.uint8)
    assert dchess.pgn_movetext(mv, san3, dchess.GO_ONGOING, 1, 0) == "1. e5 Bb5 *"


def test_movetext_all_results_and_empty_game():
    mv = np.array(M.line("e2e4"), np.uint16)
    san = np.array([M.P], np.uint8)
    tokens = {dchess.GO_ONGOING: "*", dchess.GO_WHITE_WINS: "1-0", dchess.GO_BLACK_WINS: "0-1"}
    tokens.update({k: "1/2-1/2" for k in DRAWS})
    assert sorted(tokens) == list(range(dchess.GO_COUNT))
    none = np.zeros(0, np.uint16), np.zeros(0, np.uint8)
    for k, tok in tokens.items():
        assert dchess.pgn_movetext(mv, san, k) == "1. e4 " + tok
        assert dchess.pgn_movetext(none[0], none[1], k) == tok  # a game with no moves
        assert dchess.pgn_movetext(mv, np.array([0xFF], np.uint8), k) == tok  # ... or none accepted
        r, n, text = raw_movetext(None, None, 0, 1, 1, 0, k, 16)
        assert (r, text) == (0, tok)
    assert S.RESULT_TOKEN == tokens


def test_movetext_stride_picks_a_column():
    games = [M.line("f2f3 e7e5 g2g4 d8h4"), M.line("e2e5 g1f3 d7d5"), M.line("e2e4")]
    n = max(len(g) for g in games)
    mv = np.full((n, 3), 0xFFFF, np.uint16)
    san = np.full((n, 3), 0xFF, np.uint8)
    want = []
    for g, line in enumerate(games):
        r = S.annotate(line)
        mv[:len(line), g] = line
        san[:len(line), g] = r["san"]
        want.append(S.movetext(line, r["san"], r["result"]))
    assert want == ["1. f3 e5 2. g4 Qh4# 0-1", "1. Nf3 d5 *", "1. e4 *"]
    for g in range(3):
        res = [dchess.GO_BLACK_WINS, dchess.GO_ONGOING, dchess.GO_ONGOING][g]
        col_m, col_s = mv.reshape(-1)[g:], san.reshape(-1)[g:]
        r, size, _ = raw_movetext(col_m, col_s, n, 3, 1, 0, res, 0)
        assert r == 0
        r, size2, text = raw_movetext(col_m, col_s, n, 3, 1, 0, res, size + 1)
        assert (r, size2, text) == (0, size, want[g])
    # stride 0 reads as 1, like dc_history_append
    r, _, text = raw_movetext(mv[:, 0].copy(), san[:, 0].copy(), n, 0, 1, 0, dchess.GO_BLACK_WINS, 64)
    assert (r, text) == (0, want[0])


def test_movetext_sizing_contract_and_errors():
    mv = np.array(M.line("f2f3 e7e5 g2g4 d8h4"), np.uint16)
    san = np.array(S.annotate(mv)["san"], np.uint8)
    want = "1. f3 e5 2. g4 Qh4# 0-1"
    r, size, _ = raw_movetext(mv, san, 4, 1, 1, 0, dchess.GO_BLACK_WINS, 0)
    assert (r, size) == (0, len(want))  # out_cap 0 only sizes
    r, size, text = raw_movetext(mv, san, 4, 1, 1, 0, dchess.GO_BLACK_WINS, len(want) + 1)
    assert (r, size, text) == (0, len(want), want)
    for cap in (1, len(want)):  # too small (the NUL needs room): the length is still reported
        r, size, _ = raw_movetext(mv, san, 4, 1, 1, 0, dchess.GO_BLACK_WINS, cap)
        assert (r, size) == (dchess.EINVAL, len(want))
    L = dchess.lib()
    n = C.c_size_t()
    buf = C.create_string_buffer(64)
    assert L.dc_pgn_movetext(None, dchess._ptr(san), 4, 1, 1, 0, 0, buf, 64, C.byref(n)) == dchess.EINVAL
    assert L.dc_pgn_movetext(dchess._ptr(mv), None, 4, 1, 1, 0, 0, buf, 64, C.byref(n)) == dchess.EINVAL
    assert L.dc_pgn_movetext(dchess._ptr(mv), dchess._ptr(san), 4, 1, 1, 0, 0, buf, 64, None) == dchess.EINVAL
    assert L.dc_pgn_movetext(dchess._ptr(mv), dchess._ptr(san), 4, 1, 1, 0, 0, None, 64, C.byref(n)) == dchess.EINVAL
    assert L.dc_pgn_movetext(dchess._ptr(mv), dchess._ptr(san), 4, 1, 1, 2, 0, buf, 64, C.byref(n)) == dchess.EINVAL
    assert L.dc_pgn_movetext(dchess._ptr(mv), dchess._ptr(san), 4, 1, 1, 0, dchess.GO_COUNT, buf, 64,
                             C.byref(n)) == dchess.EINVAL
    bad = san.copy()
    bad[1] = 6  # a byte no move has
    assert L.dc_pgn_movetext(dchess._ptr(mv), dchess._ptr(bad), 4, 1, 1, 0, 0, buf, 64, C.byref(n)) == dchess.EINVAL


def golden_fens():
    fens = set()

    def walk(x):
        if isinstance(x, dict):
            for k, v in x.items():
                if k == "fen" and isinstance(v, str):
                    fens.add(v)
                walk(v)
        elif isinstance(x, list):
            for v in x:
                walk(v)

    for f in sorted(os.listdir(GOLDEN)):
        if f.endswith(".json"):
            walk(json.load(open(os.path.join(GOLDEN, f))))
    return sorted(fens)


def test_pos_to_fen_round_trip():
    fens = golden_fens()
    assert len(fens) >= 6
    fens += sorted({l[0] for l in LINES if l[0]} | {p[1] for p in PINNED if p[1]})
    fens += ["r3k2r/8/8/8/8/8/8/R3K2R b Kq e3 37 112", "8/8/8/8/k3p2Q/8/3P4/3K4 w - - 149 300",
             "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"]
    for fen in fens:
        pos = dchess.pos_from_fen(fen)
        hm, fm = dchess.fen_clocks(fen)
        text = dchess.pos_to_fen(pos, hm, fm)
        if len(fen.split()) == 6:
            assert text == " ".join(fen.split()), fen
        back = dchess.pos_from_fen(text)
        assert back.tobytes() == pos.tobytes(), fen
        assert dchess.fen_clocks(text) == (hm, fm), fen
    assert dchess.pos_to_fen(dchess.startpos()) == "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"
    assert dchess.pos_to_fen(dchess.startpos(), 4294967295, 4294967295).endswith(" 4294967295 4294967295")


def test_pos_to_fen_sizing_and_errors():
    L = dchess.lib()
    p = np.array([dchess.startpos()], dchess.POS_DTYPE)
    want = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"
    n = C.c_size_t(777)
    assert L.dc_pos_to_fen(dchess._ptr(p), 0, 1, None, 0, C.byref(n)) == 0 and n.value == len(want)
    buf = C.create_string_buffer(len(want) + 1)
    assert L.dc_pos_to_fen(dchess._ptr(p), 0, 1, buf, len(want), C.byref(n)) == dchess.EINVAL and n.value == len(want)
    assert L.dc_pos_to_fen(dchess._ptr(p), 0, 1, buf, len(want) + 1, C.byref(n)) == 0 and buf.value.decode() == want
    assert L.dc_pos_to_fen(None, 0, 1, buf, 64, C.byref(n)) == dchess.EINVAL
    assert L.dc_pos_to_fen(dchess._ptr(p), 0, 1, buf, 64, None) == dchess.EINVAL
    assert L.dc_pos_to_fen(dchess._ptr(p), 0, 1, None, 64, C.byref(n)) == dchess.EINVAL
    for field, value in (("stm", 2), ("stm", 255), ("ep", -2), ("ep", 64), ("ep", 127), ("ep", -128)):
        q = p.copy()
        q[0][field] = value
        assert L.dc_pos_to_fen(dchess._ptr(q), 0, 1, buf, 64, C.byref(n)) == dchess.EINVAL, (field, value)
    for ok in (-1, 0, 63):
        q = p.copy()
        q[0]["ep"] = ok
        assert L.dc_pos_to_fen(dchess._ptr(q), 0, 1, None, 0, C.byref(n)) == 0
    # a piece of kind OTHER has no FEN letter
    cells = O.startpos_cells().copy()
    cells[27] = 6
    other = dchess.pos_from_cells(cells, 0)
    with pytest.raises(dchess.DChessError) as e:
        dchess.pos_to_fen(other)
    assert e.value.status == dchess.EUNSUPPORTED


def test_replay_san_null_context_is_einval():
    """(The NULL-pointer cases need a context, so a device: tests/test_gpu_san.py.)"""
    L = dchess.lib()
    out = np.zeros(1, dchess.OUTCOME_DTYPE)
    mv = np.zeros(1, np.uint16)
    san = np.zeros(1, np.uint8)
    for fn in (L.dc_replay_san, L.dc_replay_san_device):
        assert fn(None, None, 0, dchess._ptr(mv), 1, 1, dchess._ptr(out), dchess._ptr(san), None, None, None,
                  None) == dchess.EINVAL


def test_games_pgn_tool_text():
    """tools/games_pgn.py's PGN of one game: the Result tag, SetUp/FEN only with a
    start FEN, a comment naming a termination that is not a mate."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("games_pgn", os.path.join(ROOT, "tools", "games_pgn.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    out = np.zeros(1, dchess.OUTCOME_DTYPE)

    def text(name, fen_tag=None):
        _, fen, hm, moves, _ = next(p for p in PINNED if p[0] == name)
        start = O.Pos.from_fen(fen) if fen else None
        mv = np.array(M.line(moves), np.uint16)
        r = S.annotate(mv, start, hm)
        out[0]["result"] = r["result"]
        return tool.pgn(mv, np.array(r["san"], np.uint8), out[0], fen_tag, 1, start.stm if start else 0)

    assert text("fools_mate_plus_one") == '[Result "0-1"]\n\n1. f3 e5 2. g4 Qh4# 0-1\n'
    assert text("seventyfive_at_start") == ('[Result "1/2-1/2"]\n\n{seventy-five moves without a pawn move or capture} '
                                            '1/2-1/2\n')
    assert text("fifty_is_a_claim") == '[Result "*"]\n\n1. Nf3 Nf6 2. Ng1 {unfinished} *\n'
    fen = "4k3/8/8/8/8/8/8/4K2R w - - 0 1"
    assert text("dead_after_capture", fen) == (f'[Result "1/2-1/2"]\n[SetUp "1"]\n[FEN "{fen}"]\n\n1. Rh8+ Kf7 2. Rh7+ '
                                               'Kg8 3. Rg7+ Kxg7 {dead position (insufficient material)} 1/2-1/2\n')
