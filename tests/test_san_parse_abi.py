"""CPU test of the host parsers dc_san_parse and dc_pgn_parse_movetext (no
device): every string dc_san_format writes over the seeded batches parses to
the token built here from its move word and SAN byte; long forms, digit-zero
castles and annotation suffixes parse; a list of rejects is DC_EINVAL; the
pinned games' movetext parses back to its tokens, result and first move
number; a hand-written text with comments, NAGs, nested variations and two
games walks correctly; sizing, a capacity that is too small and the offset of
a bad word follow the header's contract."""
import ctypes as C

import numpy as np
import pytest

import dchess
import oracle_lib as O
import outcome_model as M
import san_model as S
import san_resolve_model as R
from test_outcome_model import PINNED
from test_san_model import MOVETEXT


def token_of(m, b):
    """The token of an accepted move from its move word and SAN byte, field by field."""
    f, t, promo, kind = m & 63, (m >> 6) & 63, (m >> 12) & 7, b & 7
    suffix = R.MATE if b & S.MATE else R.CHECK if b & S.CHECK else 0
    if kind == R.K and (f >> 3) == (t >> 3) and abs((f & 7) - (t & 7)) == 2:
        return (R.OO if t > f else R.OOO) | suffix
    capture = bool(b & S.CAPTURE)
    file = (f & 7) if (b & S.FILE or (kind == R.P and capture)) else None
    rank = (f >> 3) if b & S.RANK else None
    return R.token(t, kind, promo, file, rank, capture) | suffix


@pytest.mark.parametrize("noise", [0, 32])
def test_everything_the_formatter_writes_parses(noise):
    moves, san, tokens = R.seeded(noise)
    ok = san != S.NONE
    pairs = np.unique(moves[ok].astype(np.uint32) | (san[ok].astype(np.uint32) << 16))
    assert len(pairs) > 1000
    for v in pairs.tolist():
        m, b = v & 0xFFFF, v >> 16
        text = dchess.san_format(m, b)
        assert text == S.san_text(m, b)
        assert dchess.san_parse(text) == token_of(m, b) == R.parse(text), text


def test_forms():
    P = dchess.san_parse
    assert P("e4") == R.token("e4")
    assert P("Ng1f3") == R.token("f3", R.N, file=6, rank=0)
    assert P("e2e4") == R.token("e4", R.P, file=4, rank=1)
    assert P("Qh4xe1#") == R.token("e1", R.Q, file=7, rank=3, x=True, mate=True)
    assert P("R1a2") == R.token("a2", R.R, rank=0)
    assert P("exd8=Q+") == R.token("d8", R.P, promo=4, file=4, x=True, check=True)
    assert P("a1=N") == R.token("a1", R.P, promo=1)
    assert P("e7=Q") == R.token("e7", R.P, promo=4)  # the resolver's business, not the parser's
    assert P("bxc3") == R.token("c3", R.P, file=1, x=True)
    assert P("Bxc3") == R.token("c3", R.B, x=True)
    assert P("O-O") == P("0-0") == P("O-0") == R.OO
    assert P("O-O-O") == P("0-0-0") == R.OOO
    assert P("O-O+") == R.OO | R.CHECK and P("0-0-0#") == R.OOO | R.MATE
    for suffix in ("!", "?", "!!", "??", "!?", "?!"):
        assert P("Nf3" + suffix) == R.token("f3", R.N)
        assert P("Qxf7#" + suffix) == R.token("f7", R.Q, x=True, mate=True)
        assert P("O-O" + suffix) == R.OO
    assert P(b"Kf1") == R.token("f1", R.K)


REJECTS = ["", " ", "e", "4", "e9", "i4", "Ne", "N", "x", "Nx", "exd", "e4e", "e4 ", " e4", "e.p.", "exd6e.p.",
           "exd6 e.p.", "Qe8=Q", "Nf3=N", "e8=", "e8=K", "e8=P", "e8=q", "e8Q", "Pe4", "ne4", "o-o", "O-", "O-O-",
           "O-OO", "O-O-O-O", "OO", "0-0-", "e4+#", "e4#+", "e4++", "e4!+", "Nf3\0", "--", "Z0", "1-0", "*", "12.",
           "Nbb", "Nb1d", "N1b1d2", "Nbxd", "exx4", "K", "e4=", "=Q", "+", "#", "!"]


@pytest.mark.parametrize("text", REJECTS, ids=[repr(t) for t in REJECTS])
def test_rejects(text):
    with pytest.raises(dchess.DChessError) as e:
        dchess.san_parse(text)
    assert e.value.status == dchess.EINVAL


def test_null_arguments():
    L = dchess.lib()
    tok, n = C.c_uint32(77), C.c_uint32(77)
    assert L.dc_san_parse(None, 2, C.byref(tok)) == dchess.EINVAL
    assert L.dc_san_parse(b"e4", 2, None) == dchess.EINVAL
    assert L.dc_san_parse(b"e4", 0, C.byref(tok)) == dchess.EINVAL and tok.value == 77
    assert L.dc_san_parse(b"e4xx", 2, C.byref(tok)) == 0 and tok.value == R.token("e4")  # len bounds the read
    assert L.dc_pgn_parse_movetext(b"e4", 2, None, 1, 0, None, None, None, None, None) == dchess.EINVAL
    assert L.dc_pgn_parse_movetext(None, 2, None, 1, 0, C.byref(n), None, None, None, None) == dchess.EINVAL
    assert L.dc_pgn_parse_movetext(None, 0, None, 1, 0, C.byref(n), None, None, None, None) == 0 and n.value == 0
    assert L.dc_pgn_parse_movetext(b"1. e4 e5 *", 10, None, 1, 0, C.byref(n), None, None, None, None) == 0
    assert n.value == 2


RESULT = {M.ONGOING: 0, M.WHITE_WINS: 1, M.BLACK_WINS: 2, M.STALEMATE: 3, M.DEAD: 3, M.FIVEFOLD: 3, M.SEVENTYFIVE: 3}


@pytest.mark.parametrize("name,fen,halfmove,moves,want", PINNED, ids=[p[0] for p in PINNED])
def test_pinned_movetext_parses_back(name, fen, halfmove, moves, want):
    """dc_pgn_movetext's line for a pinned game (the text pinned in test_san_model.py)
    -> the tokens of its accepted moves, its result and its first move number."""
    start = O.Pos.from_fen(fen) if fen else None
    line = np.array(M.line(moves), np.uint16)
    r = S.annotate(line, start, halfmove)
    stm = start.stm if start is not None else 0
    text = dchess.pgn_movetext(line, np.array(r["san"], np.uint8), r["result"], 1, stm)
    assert text == MOVETEXT[name]
    tokens, result, fullmove, first_stm, consumed = dchess.pgn_parse_movetext(text)
    played = [(int(m), b) for m, b in zip(line, r["san"]) if b != S.NONE]
    assert tokens.tolist() == [token_of(m, b) for m, b in played]
    assert (result, fullmove, consumed) == (RESULT[r["result"]], 1, len(text))
    assert first_stm == (stm if played else 0)  # a game without moves has no move number
    assert dchess.PGN_DRAW == 3 and (dchess.GO_ONGOING, dchess.GO_WHITE_WINS, dchess.GO_BLACK_WINS) == (0, 1, 2)


GAME_A = """1. e4 {king's pawn; a ) and a ( in a comment} e5 $1 2. Nf3 ; the rest of the line: Qh5?? 1-0
 (2. f4 exf4 (2... d5 {nested ( twice} 3. exd5) 3. Nf3 $14) 2... Nc6 3.Bb5 a6!? 4. Ba4 Nf6 5. O-O Be7
1/2-1/2"""
GAME_B = """
17... Rxe1+ 18. Qxe1 $2 {loses} ( 18. Rxe1 ) Qh4e1# 0-1 trailing words are the next game's"""


def test_hand_written_text_and_a_stream_of_games():
    text = GAME_A + GAME_B
    t, result, fullmove, stm, used = dchess.pgn_parse_movetext(text)
    assert t.tolist() == [R.parse(s) for s in "e4 e5 Nf3 Nc6 Bb5 a6 Ba4 Nf6 O-O Be7".split()]
    assert (result, fullmove, stm, used) == (dchess.PGN_DRAW, 1, 0, len(GAME_A))
    t, result, fullmove, stm, used2 = dchess.pgn_parse_movetext(text[used:])
    assert t.tolist() == [R.parse(s) for s in "Rxe1+ Qxe1 Qh4e1#".split()]
    assert (result, fullmove, stm) == (2, 17, 1)
    assert text[used + used2:] == " trailing words are the next game's"
    # the end of the text without a result, "*", a number glued to its move, no number at all
    assert dchess.pgn_parse_movetext("1. d4 d5 2. c4")[1:] == (0, 1, 0, 14)
    t, result, fullmove, stm, used = dchess.pgn_parse_movetext("5.d4 d5 * 1. e4")
    assert t.tolist() == [R.parse("d4"), R.parse("d5")] and (result, fullmove, stm, used) == (0, 5, 0, 9)
    assert dchess.pgn_parse_movetext("d4 d5 2. c4 1-0")[1:] == (1, 1, 0, 15)
    assert dchess.pgn_parse_movetext("")[1:] == (0, 1, 0, 0) and dchess.pgn_parse_movetext("  * ")[1:] == (0, 1, 0, 3)
    # an unterminated comment or variation runs to the end of the text
    assert dchess.pgn_parse_movetext("1. e4 {no end 1-0")[0].tolist() == [R.parse("e4")]
    assert dchess.pgn_parse_movetext("1. e4 (1. d4 (1. c4) 1-0")[1:] == (0, 1, 0, 24)


def _raw(text, tokens, stride, cap):
    n, res, ff, fs, used = C.c_uint32(99), C.c_uint8(99), C.c_uint32(99), C.c_uint8(99), C.c_size_t(99)
    st = dchess.lib().dc_pgn_parse_movetext(text, len(text), dchess._ptr(tokens), stride, cap, C.byref(n),
                                            C.byref(res), C.byref(ff), C.byref(fs), C.byref(used))
    return st, n.value, res.value, ff.value, fs.value, used.value


def test_sizing_and_capacity():
    text = b"3... Nf6 4. Ng5 d5 5. exd5 0-1"
    want = [R.parse(s) for s in "Nf6 Ng5 d5 exd5".split()]
    buf = np.full(12, 0xAAAAAAAA, np.uint32)
    assert _raw(text, None, 1, 8) == (0, 4, 2, 3, 1, len(text))       # tokens NULL: sizes only
    assert _raw(text, buf, 1, 0) == (0, 4, 2, 3, 1, len(text))        # cap 0: sizes only
    assert (buf == 0xAAAAAAAA).all()
    assert _raw(text, buf, 1, 4) == (0, 4, 2, 3, 1, len(text)) and buf.tolist() == want + [0xAAAAAAAA] * 8
    buf[:] = 0xAAAAAAAA
    assert _raw(text, buf, 3, 4) == (0, 4, 2, 3, 1, len(text))        # a column of a [n][3] array
    assert buf[0::3].tolist() == want and (buf.reshape(4, 3)[:, 1:] == 0xAAAAAAAA).all()
    buf[:] = 0xAAAAAAAA
    assert _raw(text, buf, 1, 3) == (dchess.EINVAL, 4, 2, 3, 1, len(text))  # too small: the size, nothing past cap
    assert buf.tolist() == want[:3] + [0xAAAAAAAA] * 9
    buf[:] = 0xAAAAAAAA
    assert _raw(text, buf, 0, 4)[0] == 0 and buf[:4].tolist() == want  # stride 0 counts as 1


def test_a_bad_word_is_reported_at_its_offset():
    text = "1. e4 e5 2. Nf3 Nc9 3. Bb5 1-0"
    with pytest.raises(dchess.DChessError) as e:
        dchess.pgn_parse_movetext(text)
    assert e.value.status == dchess.EINVAL and e.value.offset == text.index("Nc9")
    raw = text.encode()
    buf = np.full(8, 0xAAAAAAAA, np.uint32)
    st, n, _, ff, fs, used = _raw(raw, buf, 1, 8)
    assert (st, n, ff, fs, used) == (dchess.EINVAL, 3, 1, 0, raw.index(b"Nc9"))
    assert buf[:3].tolist() == [R.parse(s) for s in ("e4", "e5", "Nf3")] and (buf[3:] == 0xAAAAAAAA).all()
    for bad in ("1. e4 e.p. 1-0", "1. e4 ) e5", "1. e4 [Event", "1. e4 1-1", "1. e4 e5 2.. x"):
        with pytest.raises(dchess.DChessError):
            dchess.pgn_parse_movetext(bad)


def test_pgn_games_splits_tags_and_movetext():
    text = ('[Event "a \\"quoted\\" name"]\n[Result "1-0"]\n\n1. e4 e5\n2. Nf3 1-0\n\n'
            '[Event "second"]\n[FEN "4k3/8/8/8/8/8/8/4K3 w - - 0 1"]\n\n1. Kd1 *\n\n1. e4 *\n')
    games = dchess.pgn_games(text)
    assert games == [({"Event": 'a "quoted" name', "Result": "1-0"}, "1. e4 e5\n2. Nf3 1-0"),
                     ({"Event": "second", "FEN": "4k3/8/8/8/8/8/8/4K3 w - - 0 1"}, "1. Kd1 *\n\n1. e4 *")]
    assert dchess.pgn_games("") == [] and dchess.pgn_games("1. e4 *") == [({}, "1. e4 *")]
