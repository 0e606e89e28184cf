"""The board's symmetries, as maps on everything the rules calls take and
return -- TEST INFRASTRUCTURE ONLY.

  F  colour flip   square s -> s ^ 56, every piece changes colour, stm ^= 1,
                   castle bits (0,1) <-> (2,3), ep -> ep ^ 56
  M  file mirror   square s -> s ^ 7, colours and stm kept, ep -> ep ^ 7
  R  = F o M       square s -> s ^ 63

Chess under both rule sets is invariant under all three, except that castling
is not mirror-symmetric (the king stands on the e-file, not the d-file): M and
R take positions with castle == 0 only and raise on any other; a caller clears
the rights first with without_rights(), on both sides of its comparison.
I is the identity, for code that treats an unmapped column like the others.

Each map is an involution, so a table indexed by move word is read back through
the same map: verdicts_of_T_x[T.words4096()] are x's verdicts in x's order,
whether the table is indexed by word (from | to << 6) or, as the oracles' are,
by 64 * from + to -- the same xor maps both.

The second half builds the game batch that tests/test_symmetry_model.py and
tests/test_gpu_symmetry.py share: every game five times (as it is, under F,
with the rights cleared, and that under M and R), and the models' answers for
the two unmapped columns.  Nothing here touches the GPU.
"""
import functools

import numpy as np

import oracle_lib as O

NONE = 0xFFFF
TOKEN_NONE = 0xFFFFFFFF
GO_WHITE_WINS, GO_BLACK_WINS = 1, 2


def without_rights(p):
    """The position with its castling rights cleared (an oracle Pos or a dc_pos record)."""
    if isinstance(p, O.Pos):
        return O.Pos(p.cells.copy(), p.stm, 0, p.ep)
    q = p.copy()
    q["castle"] = 0
    return q


class Sym:
    def __init__(self, name, xor):
        self.name, self.xor = name, xor
        self.flips_colour = bool(xor & 56)
        self.mirrors_files = bool(xor & 7)

    def __repr__(self):
        return self.name

    # ------------------------------------------------------------- squares
    def sq(self, s):
        return s ^ self.xor

    # ----------------------------------------------------------- positions
    def _fields(self, cells, stm, castle, ep):
        if self.mirrors_files and castle:
            raise ValueError("%s: castling rights are not mirror-symmetric; clear them first" % self.name)
        cells = np.asarray(cells, np.int8)
        out = np.full(64, -1, np.int8)
        src = cells[np.arange(64) ^ self.xor]
        out[:] = np.where(src >= 0, src ^ 8, src) if self.flips_colour else src
        if self.flips_colour:
            stm ^= 1
            castle = ((castle & 3) << 2) | ((castle >> 2) & 3)
        return out, stm, castle, (ep ^ self.xor) if ep >= 0 else ep

    def pos(self, p):
        """An oracle Pos, a dc_pos record or an array of dc_pos records, mapped."""
        if isinstance(p, O.Pos):
            return O.Pos(*self._fields(p.cells, p.stm, p.castle, p.ep))
        import dchess
        if isinstance(p, np.ndarray) and p.ndim:
            return np.array([self.pos(r) for r in p.reshape(-1)], dchess.POS_DTYPE).reshape(p.shape)
        cells, turn = dchess.pos_to_cells(p)
        cells, stm, castle, ep = self._fields(cells, int(turn), int(p["castle"]), int(p["ep"]))
        d = dchess.pos_from_cells(cells, stm)
        d["castle"], d["ep"] = castle, ep
        return d

    # ---------------------------------------------------------- move words
    def moves(self, words):
        """from and to mapped, the promotion bits 12-14 kept; a word with bit 15
        set (DC_MOVE_NONE among them) is left as it is.  An int gives an int,
        an array an array of its shape, anything else a list of ints."""
        a = np.asarray(words).astype(np.int64)
        out = np.where(a & 0x8000, a, a ^ (self.xor | (self.xor << 6)))
        if isinstance(words, np.ndarray):
            return out.astype(np.uint16)
        return int(out) if out.ndim == 0 else [int(w) for w in out]

    def words4096(self):
        """The images of the 4,096 plain words from | to << 6, in word order."""
        return self.moves(np.arange(4096, dtype=np.uint16)).astype(np.int64)

    def canonical(self, words):
        """A mapped move list back in (from, to, promo) order."""
        out = sorted((int(w) for w in words), key=lambda m: (m & 63, (m >> 6) & 63, m >> 12))
        return np.array(out, np.uint16) if isinstance(words, np.ndarray) else out

    def divide(self, d):
        """A divide {root move: count} with its keys mapped (str keys stay str)."""
        return {(str(self.moves(int(k))) if isinstance(k, str) else self.moves(int(k))): v for k, v in d.items()}

    # --------------------------------------------------------- token words
    def tokens(self, words):
        """dc_san_resolve token words: the target square mapped, the origin file
        under M and R where it is given (bit 12), the origin rank under F and R
        where it is given (bit 16).  Castle tokens, malformed tokens and
        DC_SAN_TOKEN_NONE are left as they are."""
        import san_resolve_model as SR
        a = np.asarray(words).astype(np.int64)
        uniq = np.unique(a)
        fixed = np.array([int(t) == TOKEN_NONE or SR.malformed(int(t)) or bool((int(t) >> 20) & 3) for t in uniq], bool)
        keep = fixed[np.searchsorted(uniq, a)]
        out = a ^ self.xor
        if self.mirrors_files:
            out = np.where(a & SR.FILE_GIVEN, out ^ (7 << 13), out)
        if self.flips_colour:
            out = np.where(a & SR.RANK_GIVEN, out ^ (7 << 17), out)
        out = np.where(keep, a, out)
        if isinstance(words, np.ndarray):
            return out.astype(np.uint32)
        return int(out) if out.ndim == 0 else [int(w) for w in out]

    # -------------------------------------------------------------- results
    def result(self, code):
        """A DC_GO_* code: the two wins change places under F and R."""
        if self.flips_colour and code in (GO_WHITE_WINS, GO_BLACK_WINS):
            return GO_WHITE_WINS + GO_BLACK_WINS - code
        return code


I, F, M, R = Sym("I", 0), Sym("F", 56), Sym("M", 7), Sym("R", 63)
ALL = (F, M, R)


def images(p):
    """[(T, the position that T takes, T of it)] for F, M and R: M and R take p with its rights cleared."""
    p0 = without_rights(p)
    return [(F, p, F.pos(p)), (M, p0, M.pos(p0)), (R, p0, R.pos(p0))]


# ---------------------------------------------------------------- the game batch
N_PLIES = 400
PER_BATCH = 64
COLUMNS = (I, F, I, M, R)          # per game: g, F(g), g without rights, M and R of that
BASE_OF = (0, 0, 1, 1, 1)          # ... and which of the game's two unmapped columns each is the image of
JUNK_SEED = 2026
JUNK_SHARE = 0.02
THREE_QUEENS = "8/k7/8/8/7Q/8/8/K3Q2Q w - - 0 1"


def M_line(text):
    import outcome_model
    return outcome_model.line(text)


@functools.lru_cache(maxsize=None)
def games():
    """[(move words [N_PLIES], start Pos, half-move clock)]: the first 64 columns of
    fide_replay_batches.BIG (long games from the start position), the first 64 of
    SHARDED (an eighth of their words junk), starts_batches.mixed() and one constructed line."""
    import fide_replay_batches as FB
    import starts_batches as SB
    out = []

    def column(words):
        col = np.full(N_PLIES, NONE, np.uint16)
        col[:len(words)] = words
        return col

    for spec in (FB.BIG, FB.SHARDED):
        mv = FB.games(*spec)
        for g in range(PER_BATCH):
            out.append((column(mv[:, g]), O.Pos(), 0))
    b = SB.mixed()
    for g in range(b.n):
        out.append((column(b.moves[:, g]), b.starts[g], int(b.clocks[g])))
    # by construction: a move that is written with its file and its rank (three queens reach e4)
    out.append((column(M_line("h1e4 a7b8 e4h1 b8a7 h1e4")), O.Pos.from_fen(THREE_QUEENS), 3))
    return out


class Base:
    """The models' answers for one unmapped column (a game, or the game from its
    start without rights): san_model.annotate's dict, the resolver's tokens (the
    parse of the model's SAN text, then seeded junk) and san_resolve_model.walk's
    answer for them with the final position walked over the resolved words."""

    def __init__(self, moves, start, clock, rng):
        import san_model as S
        import san_resolve_model as SR
        self.moves, self.start, self.clock = moves, start, clock
        self.game = S.annotate(moves, start, clock)
        self.san = np.array(self.game["san"], np.uint8)
        tokens = np.full(len(moves), TOKEN_NONE, np.uint32)
        for p in np.flatnonzero(self.san != S.NONE):
            tokens[p] = SR.parse(S.san_text(int(moves[p]), int(self.san[p])))
        self.clean_tokens = tokens.copy()
        # junk: every third hint dropped (an ambiguous token), and over a fiftieth of the rest a
        # file that is not the origin's, a random 32-bit word or no token
        live = np.flatnonzero(tokens != TOKEN_NONE)
        for p in live:
            t = int(tokens[p])
            castle = bool(t & (SR.OO | SR.OOO))
            if not castle and (t >> 6) & 7 and t & (SR.FILE_GIVEN | SR.RANK_GIVEN) and rng.random() < 1 / 3:
                tokens[p] = t & ~(SR.FILE_GIVEN | SR.RANK_GIVEN | (7 << 13) | (7 << 17))
            elif rng.random() < JUNK_SHARE:
                how = int(rng.integers(0, 3))
                if how == 0:
                    file = (((t >> 13) & 7 if t & SR.FILE_GIVEN else t & 7) + int(rng.integers(1, 8))) & 7
                    tokens[p] = (t & ~(7 << 13)) | SR.FILE_GIVEN | (file << 13)
                else:
                    tokens[p] = int(rng.integers(0, 1 << 32)) if how == 1 else TOKEN_NONE
        self.tokens = tokens
        words, self.first_bad, self.counts = SR.walk(tokens, start)
        self.words = np.array(words, np.uint16)
        p = start.copy()
        for w in words:
            if not w & 0x8000:
                p = O.fast_make(p, int(w), O.FIDE)
        self.resolved_final = p


@functools.lru_cache(maxsize=None)
def bases():
    """[(Base of the game, Base of the game without its start's rights)] per game."""
    rng = np.random.default_rng(JUNK_SEED)
    return [(Base(mv, s, c, rng), Base(mv, without_rights(s), c, rng)) for mv, s, c in games()]


class Columns:
    """The batch: five columns per game, a game's five next to each other.  Per
    column: T (COLUMNS), base (the Base it is the image of), and the inputs
    moves [N_PLIES, n], tokens [N_PLIES, n], starts (oracle Pos), clocks."""

    def __init__(self):
        import starts_batches as SB
        self.T, self.base, self.starts, cols, toks, clocks = [], [], [], [], [], []
        for pair in bases():
            for T, k in zip(COLUMNS, BASE_OF):
                b = pair[k]
                self.T.append(T)
                self.base.append(b)
                self.starts.append(T.pos(b.start))
                cols.append(T.moves(b.moves))
                toks.append(T.tokens(b.tokens))
                clocks.append(b.clock)
        self.n = len(self.T)
        self.moves = np.ascontiguousarray(np.stack(cols, axis=1), np.uint16)
        self.tokens = np.ascontiguousarray(np.stack(toks, axis=1), np.uint32)
        self.clocks = np.array(clocks, np.uint16)
        self.dstarts = SB.pos_array(self.starts)
        # expected, mapped from the bases
        self.result = np.array([T.result(b.game["result"]) for T, b in zip(self.T, self.base)], np.uint8)
        self.end_ply = np.array([b.game["end_ply"] for b in self.base], np.uint32)
        self.repeats = np.array([b.game["repeats"] for b in self.base], np.uint8)
        self.halfmove = np.array([b.game["halfmove"] for b in self.base], np.uint16)
        self.accept = np.array([b.game["accept"] for b in self.base], bool).T
        self.san = np.stack([b.san for b in self.base], axis=1)
        self.finals = SB.pos_array([T.pos(b.game["pos"]) for T, b in zip(self.T, self.base)])
        self.counts = np.bincount(self.result, minlength=7).astype(np.uint64)
        self.validated = sum(b.game["validated"] for b in self.base)
        self.accepted = sum(b.game["accepted"] for b in self.base)
        self.bitmap = np.zeros((N_PLIES, (self.n + 63) // 64), np.uint64)
        for p, g in np.argwhere(self.accept):
            self.bitmap[p, g >> 6] |= np.uint64(1 << (int(g) & 63))
        self.words = np.stack([T.moves(b.words) for T, b in zip(self.T, self.base)], axis=1)
        self.first_bad = np.array([b.first_bad for b in self.base], np.uint32)
        self.resolve_counts = np.sum([b.counts for b in self.base], axis=0).astype(np.uint64)
        self.resolved_finals = SB.pos_array([T.pos(b.resolved_final) for T, b in zip(self.T, self.base)])


@functools.lru_cache(maxsize=None)
def columns():
    return Columns()


def batch_shape():
    """What the unmapped columns hold, for the conditions a test asserts before it
    trusts the batch: a dict of counts."""
    import san_model as S
    import san_resolve_model as SR
    out = {"results": set(), "castles": set(), "ep": 0, "promos": set(), "san": set(), "words": set()}
    for pair in bases():
        for k, b in enumerate(pair):
            out["results"].add(b.game["result"])
            out["san"] |= {int(x) & (S.FILE | S.RANK) for x in b.san[b.san != S.NONE]}
            out["words"] |= {int(w) for w in b.words if int(w) in (SR.NOMATCH, SR.AMBIGUOUS, SR.MALFORMED)}
            pos = b.start.copy()
            for ply in np.flatnonzero(b.game["accept"]):
                m = int(b.moves[ply])
                f, t = m & 63, (m >> 6) & 63
                kind = int(pos.cells[f]) & 7
                if kind == 5 and abs(t - f) == 2 and (t >> 3) == (f >> 3) and k == 0:
                    out["castles"].add((pos.stm, "k" if t > f else "q"))
                if kind == 0 and t == pos.ep and (f & 7) != (t & 7):
                    out["ep"] += 1
                if m >> 12:
                    out["promos"].add(m >> 12)
                pos = O.fast_make(pos, m, O.FIDE)
    return out
