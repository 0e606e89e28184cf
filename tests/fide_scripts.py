"""Hand-scripted FIDE games for the replay tests -- TEST INFRASTRUCTURE ONLY.

The replay's digest covers piece placement and side to move, not castling
rights or the en-passant square, so a wrong right or a stale en-passant square
after a move shows only in a later accept bit.  Each script below is a start
(a FEN, or None for the start position), a line of move words and the accept
string expected of it, written by hand from the FIDE rules:

  '1' accepted, '0' rejected, '.' a DC_MOVE_NONE ply (skipped: not counted,
  the turn does not flip).

Move text: 'e2e4'; 'a7a8=3' carries promotion code 3 (1..4 = N B R Q, 5..7
name no piece); 'e7e5!' has bit 15 set; '--' is DC_MOVE_NONE.  `castle` and
`ep` are the rights (1 K, 2 Q, 4 k, 8 q) and the en-passant square (-1 none)
after the last ply.  tests/test_fide_replay_model.py holds the oracle to these
strings; tests/test_gpu_fide_replay.py holds the kernel to them.
"""
import collections

NONE = 0xFFFF

Script = collections.namedtuple("Script", "name fen moves bits castle ep")


def sq(name):
    return 8 * (int(name[1]) - 1) + (ord(name[0]) - ord("a"))


def word(text):
    if text == "--":
        return NONE
    flag = 0x8000 if text.endswith("!") else 0
    text = text.rstrip("!")
    promo = int(text[5]) if len(text) > 4 else 0
    assert len(text) in (4, 6) and (len(text) == 4 or text[4] == "=") and 0 <= promo <= 7
    return sq(text[0:2]) | (sq(text[2:4]) << 6) | (promo << 12) | flag


def words(script):
    return [word(t) for t in script.moves.split()]


def validated(script):
    """Plies that count: every one that is not DC_MOVE_NONE."""
    return len(script.bits) - script.bits.count(".")


OPEN = "e2e4 e7e5 g1f3 b8c6 f1e2 f8e7 "  # both sides ready to castle short

START = [
    Script("castle_short", None, OPEN + "e1g1", "1111111", 12, -1),
    # the king left e1 and came back: the rights are gone, e1g1 is no castle and no king move
    Script("king_came_back", None, OPEN + "e1f1 g8f6 f1e1 f6g8 e1g1 e1f1", "111111111101", 12, -1),
    # the rook left h1 and came back: O-O lost; O-O-O still held but b1, c1, d1 are occupied; Kf1 is plain
    Script("rook_came_back", None, OPEN + "h1g1 g8f6 g1h1 f6g8 e1g1 e1c1 e1f1", "1111111111001", 12, -1),
    Script("en_passant_at_once", None, "e2e4 a7a6 e4e5 d7d5 e5d6", "11111", 15, -1),
    # one move pair later the capture is gone; the pawn may still push
    Script("en_passant_too_late", None, "e2e4 a7a6 e4e5 d7d5 a2a3 a6a5 e5d6 e5e6", "11111101", 15, -1),
    # a skipped ply does not flip the turn: Black's e7e5 is accepted, the second one finds e7 empty
    Script("none_in_the_middle", None, "e2e4 -- e7e5 e7e5 -- g1f3", "1.10.1", 15, -1),
    # a flagged word is validated and rejected whatever its low bits say; the last e2e4 has no pawn to move
    Script("flagged_word", None, "e2e4 e7e5! e7e5 e2e4", "1010", 15, 44),
    # a promotion code on a knight move and on a pawn move that does not reach the last rank
    Script("code_on_a_piece", None, "g1f3=4 g1f3 e7e5=2 e7e5", "0101", 15, 44),
]

EP_FEN = "rnbqkbnr/ppp1pppp/8/3pP3/8/8/PPPP1PPP/RNBQKBNR w KQkq %s 0 3"
ROOKS = "r3k2r/8/8/8/8/8/8/R3K2R %s %s - 0 1"
BISHOP = "r3k2r/8/8/8/8/8/6b1/R3K2R b KQkq - 0 1"
PROMO = "8/P6k/8/8/8/8/8/K7 w - - 0 1"

CUSTOM = [
    Script("start_ep_square", EP_FEN % "d6", "e5d6 d8d6", "11", 15, -1),
    Script("start_no_ep_square", EP_FEN % "-", "e5d6 e5e6", "01", 15, -1),
    # the bishop takes the h1 rook: White's O-O goes with it, O-O-O stays; then both sides castle
    Script("rook_taken_at_home", BISHOP, "g2h1 e1c1 e8g8 c1b1", "1111", 0, -1),
    Script("rook_taken_no_short", BISHOP, "g2h1 e1g1 e1c1", "101", 12, -1),
    Script("bishop_beside_the_path", BISHOP, "g2f3 e1g1", "11", 12, -1),
    # out of check: no castle either way, the king takes the checking rook
    Script("castle_out_of_check", "4k3/8/8/8/8/8/4r3/R3K2R w KQ - 0 1", "e1g1 e1c1 e1e2", "001", 0, -1),
    # through check: f1 (d1) is attacked, the other side is free; an attacked b1 does not matter
    Script("castle_through_f1", "4kr2/8/8/8/8/8/8/R3K2R w KQ - 0 1", "e1g1 e1c1", "01", 0, -1),
    Script("castle_through_d1", "3rk3/8/8/8/8/8/8/R3K2R w KQ - 0 1", "e1c1 e1g1", "01", 0, -1),
    Script("castle_past_attacked_b1", "1r2k3/8/8/8/8/8/8/R3K2R w KQ - 0 1", "e1c1", "1", 0, -1),
    # the capture would leave a4 and h4 alone on the rank; the push does not
    Script("en_passant_exposes_king", "8/8/8/8/k2Pp2Q/8/8/3K4 b - d3 0 1", "e4d3 e4e3", "01", 0, -1),
    # the pawn that just pushed gives check: pushing past it is no answer, taking it en passant is
    Script("en_passant_evades", "8/8/8/2k5/3Pp3/8/8/4K3 b - d3 0 1", "e4e3 e4d3", "01", 0, -1),
    # Black promotes: no code, a code that names no piece, then a knight by capture
    Script("black_underpromotes", "4k3/8/8/8/8/8/p7/1N2K3 b - - 0 1", "a2a1 a2b1=5 a2b1=1 e1d1", "0011", 0, -1),
]

# a7a8 with every promotion code, then Black's reply (rejected as White's move when the pawn stayed)
PROMOTIONS = [Script("promote_code_%d" % k, PROMO, "a7a8=%d h7h6" % k, "11" if 1 <= k <= 4 else "00", 0, -1)
              for k in range(8)]

_RIGHT = {"K": 1, "Q": 2, "k": 4, "q": 8}
_CASTLES = {"w": (("e1g1", "K"), ("e1c1", "Q")), "b": (("e8g8", "k"), ("e8c8", "q"))}


def _castle_scripts():
    """Kings and rooks at home, one castle a game: accepted exactly when the
    side to move holds that right; then its two rights are gone and the other
    side's are kept."""
    out = []
    for rights in ("K", "Q", "k", "q", "KQkq", "-"):
        held = sum(_RIGHT[c] for c in rights if c in _RIGHT)
        for side in "wb":
            for text, right in _CASTLES[side]:
                ok = right in rights
                after = held & ~(3 if side == "w" else 12) if ok else held
                out.append(Script("rights_%s_%s_%s" % (rights, side, text), ROOKS % (side, rights), text,
                                  "1" if ok else "0", after, -1))
    return out


CASTLES = _castle_scripts()
ALL = START + CUSTOM + PROMOTIONS + CASTLES


def matrix(scripts):
    """The scripts of one start as a ply-major uint16 matrix padded with DC_MOVE_NONE."""
    import numpy as np
    mv = np.full((max(len(s.bits) for s in scripts), len(scripts)), NONE, np.uint16)
    for g, s in enumerate(scripts):
        mv[:len(s.bits), g] = words(s)
    return mv


def column_bits(bitmap, mv, g, n):
    """The first n plies of column g of an accept bitmap, in the scripts' notation."""
    return "".join("." if mv[ply, g] == NONE else str((int(bitmap[ply, g >> 6]) >> (g & 63)) & 1) for ply in range(n))


def groups():
    """The scripts that share a start, in order: [(fen or None, [scripts])]; one replay call each."""
    by = collections.OrderedDict()
    for s in ALL:
        by.setdefault(s.fen, []).append(s)
    return list(by.items())
