"""The inputs and expected values of the per-game-start tests (dc_replay_outcome_starts,
dc_replay_san_starts, dc_san_resolve_starts) -- TEST INFRASTRUCTURE ONLY.

One mixed batch: the games of fide_replay_batches.games_from(i) for every custom
start i, interleaved so that neighbouring lanes have different starts, with a
clock per game from CLOCKS, then constructed lines that put every class of game
into the batch by construction.  Expected values come from the oracle-backed
models, ONE CALL PER GAME with that game's own start and clock
(san_model.annotate, san_resolve_model.walk); the final positions are walked
with oracle_lib.fast_make.  Nothing here touches the GPU;
tests/test_starts_model.py asserts what the batch holds.
"""
import functools

import numpy as np

import dchess
import fide_replay_batches as FB
import oracle_lib as O
import outcome_model as M
import san_model as S
import san_resolve_model as R

NONE = 0xFFFF
CLOCKS = (0, 1, 99, 134, 140, 149, 150)
PER_START = 8     # games taken from every custom start
SEEDED_PLIES = 30
N_PLIES = 40
SHUFFLE = M.line("g1f3 g8f6 f3g1 f6g8") * 10  # 40 plies; the start position recurs every 4
MATE_FEN = "rnb1kbnr/pppp1ppp/8/4p3/6Pq/5P2/PPPPP2P/RNBQKBNR w KQkq - 1 3"
STALE_FEN = "7k/5Q2/6K1/8/8/8/8/8 b - - 0 1"
DEAD_FEN = "4k3/8/8/8/8/8/8/4K3 w - - 0 1"
LEGAL_LOOKING = M.line("e1e2 e8e7 a2a3 h8g8")


def dpos(p):
    """oracle Pos -> dc_pos record."""
    d = dchess.pos_from_cells(p.cells, p.stm)
    d["castle"], d["ep"] = p.castle, p.ep
    return d


def pos_array(ps):
    return np.array([dpos(p) for p in ps], dchess.POS_DTYPE)


def same_pos(a, b):
    """Element-wise equality of two dc_pos arrays, reserved fields included."""
    return a.view(np.uint8).reshape(len(a), 40) == b.view(np.uint8).reshape(len(b), 40)


class Batch:
    """starts: [oracle Pos]; clocks: uint16 [n]; moves: uint16 [n_plies, n]; label: [str]."""

    def __init__(self, starts, clocks, moves, labels):
        self.starts, self.labels = list(starts), list(labels)
        self.clocks = np.array(clocks, np.uint16)
        self.moves = np.ascontiguousarray(moves, np.uint16)
        self.n = len(self.starts)
        assert self.moves.shape[1] == self.n == len(self.clocks)
        self.dstarts = pos_array(self.starts)

    def take(self, idx):
        idx = list(idx)
        return Batch([self.starts[i] for i in idx], self.clocks[idx], self.moves[:, idx], [self.labels[i] for i in idx])


def _column(words, n_plies=N_PLIES):
    col = np.full(n_plies, NONE, np.uint16)
    col[:len(words)] = words[:n_plies]
    return col


@functools.lru_cache(maxsize=None)
def mixed():
    cs = FB.custom_starts()
    starts, clocks, cols, labels = [], [], [], []
    for j in range(PER_START):
        for i, (label, p) in enumerate(cs):  # neighbouring lanes: different starts
            starts.append(p)
            clocks.append(CLOCKS[len(cols) % len(CLOCKS)])
            cols.append(_column(FB.games_from(i, PER_START, SEEDED_PLIES)[:, j]))
            labels.append(label)
    # by construction: the knight shuffle from the start position at every clock
    # (fivefold from 0, 1, 99 and 134, seventy-five from 140, 149 and 150) ...
    for hm in CLOCKS:
        starts.append(O.Pos())
        clocks.append(hm)
        cols.append(_column(SHUFFLE))
        labels.append("shuffle_%d" % hm)
    # ... and starts that are already over
    for name, fen in (("mate", MATE_FEN), ("stalemate", STALE_FEN), ("dead", DEAD_FEN)):
        starts.append(O.Pos.from_fen(fen))
        clocks.append(dchess.fen_clocks(fen)[0])
        cols.append(_column(LEGAL_LOOKING))
        labels.append("start_" + name)
    return Batch(starts, clocks, np.stack(cols, axis=1), labels)


def shuffle_wave():
    """One wave: the knight shuffle from the start position at every clock of CLOCKS, repeated to 64 lanes."""
    hms = [CLOCKS[k % len(CLOCKS)] for k in range(64)]
    return Batch([O.Pos()] * 64, hms, np.stack([_column(SHUFFLE)] * 64, axis=1), ["shuffle_%d" % h for h in hms])


def distinct_starts(n=257, plies=12):
    """n games with n distinct starts: seeded game g's position after g % 9 + 8 of
    its own plies, then its next plies."""
    mv = O.fast_gen_games(2024, 0, n, 17 + plies, 0, O.FIDE)
    starts, cols = [], []
    for g in range(n):
        p = O.Pos()
        k = g % 9 + 8
        for m in mv[:k, g]:
            p = O.fast_make(p, int(m), O.FIDE)
        starts.append(p)
        cols.append(_column(mv[k:k + plies, g], plies))
    return Batch(starts, [CLOCKS[g % len(CLOCKS)] for g in range(n)], np.stack(cols, axis=1), ["g%d" % g for g in range(n)])


class Expected:
    """The models' answers for a Batch, one model call per game."""

    def __init__(self, b):
        n_plies = b.moves.shape[0]
        words = (b.n + 63) // 64
        self.games = [S.annotate(b.moves[:, g], b.starts[g], int(b.clocks[g])) for g in range(b.n)]
        self.outcomes = [(r["result"], r["end_ply"], r["repeats"], r["halfmove"]) for r in self.games]
        self.san = np.array([r["san"] for r in self.games], np.uint8).T.reshape(n_plies, b.n)
        self.bitmap = np.zeros((n_plies, words), np.uint64)
        for g, r in enumerate(self.games):
            for ply, ok in enumerate(r["accept"]):
                if ok:
                    self.bitmap[ply, g >> 6] |= np.uint64(1 << (g & 63))
        self.counts = [sum(1 for r in self.games if r["result"] == k) for k in range(7)]
        val, acc = sum(r["validated"] for r in self.games), sum(r["accepted"] for r in self.games)
        self.digests = np.array([O.digest(r["pos"].cells, r["pos"].stm) for r in self.games], np.uint64)
        self.stats = {"validated": val, "accepted": acc, "rejected": val - acc,
                      "digest_sum": int(self.digests.sum(dtype=np.uint64)),
                      "digest_xor": int(np.bitwise_xor.reduce(self.digests)) if b.n else 0}
        self.finals = pos_array([r["pos"] for r in self.games])


class ExpectedResolve:
    """Tokens from the model's SAN text of the accepted plies (as san_resolve_model.seeded
    builds them); every other rejected ply holds the token of the game's first accepted
    move instead of NONE, so that flagged words occur and a few games leave the line that
    was played; the resolver model's answers, one call per game, and the
    final positions walked with fast_make over the resolved words."""

    def __init__(self, b, exp):
        n_plies = b.moves.shape[0]
        self.tokens = np.full((n_plies, b.n), R.NONE, np.uint32)
        k = 0
        for g in range(b.n):
            first = None
            for p in range(n_plies):
                byte = int(exp.san[p, g])
                if byte != S.NONE:
                    self.tokens[p, g] = R.parse(S.san_text(int(b.moves[p, g]), byte))
                    first = self.tokens[p, g] if first is None else first
                elif first is not None and int(b.moves[p, g]) != NONE and p < exp.games[g]["end_ply"]:
                    k += 1
                    if k % 2 == 0:
                        self.tokens[p, g] = first
        self.moves = np.zeros((n_plies, b.n), np.uint16)
        self.first_bad = np.zeros(b.n, np.uint32)
        self.counts = np.zeros(5, np.uint64)
        finals = []
        for g in range(b.n):
            w, fb, c = R.walk(self.tokens[:, g], b.starts[g])
            self.moves[:, g], self.first_bad[g] = w, fb
            self.counts += np.array(c, np.uint64)
            p = b.starts[g].copy()
            for m in w:
                if not m & 0x8000:
                    p = O.fast_make(p, int(m), O.FIDE)
            finals.append(p)
        self.finals = pos_array(finals)


@functools.lru_cache(maxsize=None)
def mixed_expected():
    return Expected(mixed())


@functools.lru_cache(maxsize=None)
def mixed_resolve():
    return ExpectedResolve(mixed(), mixed_expected())
