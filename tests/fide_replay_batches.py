"""The inputs of tests/test_gpu_fide_replay.py -- TEST INFRASTRUCTURE ONLY.

Every batch is named by the oracle parameters that make it
(oracle_lib.fast_gen_games under FIDE rules) or built on the host from oracle
positions with a seeded generator; nothing here touches the GPU.
tests/test_fide_replay_model.py asserts what each batch holds, so that the GPU
tests cannot pass on inputs that exercise nothing.
"""
import collections
import functools
import json
import os

import numpy as np

import fide_positions as F
import oracle_lib as O

NONE = O.SENTINEL
OG = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_golden.json")))

# (seed, first_game, n_games, n_plies, noise_per_256)
BIG = (0xF1DE, 0, 512, 400, 0)      # long games: mates and stalemates, every promotion code, castles, en passant
MID = (0xF1DE, 0, 128, 300, 0)
SHARDED = (0xF1DE, 0, 1000, 60, 32)
APPLIED = (0xF1DE, 0, 65, 40, 32)
JUNK_BASE = (0x1F1DE, 0, 200, 60, 0)
JUNK_SHARE = 0.3                     # of the plies of JUNK_BASE are overwritten
RAGGED = [(1, 1, 0), (63, 7, 32), (64, 40, 32), (65, 81, 32), (255, 30, 0), (256, 30, 0), (257, 30, 255),
          (512, 400, 0)]            # (n_games, n_plies, noise)
GEN_TABLE = [(0xF1DE, 0, 512, 400, 0), (0xF1DE, 0, 257, 600, 32), (3, 2**32 + 5, 65, 50, 256), (9, 0, 1, 300, 0),
             (11, 7, 255, 20, 255), (11, 7, 256, 20, 255)]
N_LONE = 16                          # columns of BIG replayed alone
N_FROM_SET = 24                      # custom starts taken from fide_positions.position_set(), at least


@functools.lru_cache(maxsize=None)
def games(seed, first_game, n_games, n_plies, noise):
    """The oracle's FIDE games, ply-major [n_plies, n_games]; shared, so read-only."""
    mv = O.fast_gen_games(seed, first_game, n_games, n_plies, noise_per_256=noise, rules=O.FIDE)
    mv.flags.writeable = False
    return mv


def ragged(n_games, n_plies, noise):
    if (n_games, n_plies, noise) == BIG[2:]:
        return games(*BIG)
    return games(7 + n_games, 3, n_games, n_plies, noise)


WALK_DTYPE = np.dtype([("end", "i4"), ("castle_k", "i4"), ("castle_q", "i4"), ("ep", "i4"), ("promo", "i4", (5,)),
                       ("digest", "u8")])


def walk(mv):
    """What the games of a noise-0 batch hold, game by game, from a mailbox walk
    of the move words alone (every word of such a batch is a legal move): the
    first DC_MOVE_NONE ply (n_plies when there is none), king-side and
    queen-side castles, en-passant captures, promotions by code, and the
    digest of the final board."""
    n_plies, n_games = mv.shape
    start = [int(c) for c in O.startpos_cells()]
    out = np.zeros(n_games, WALK_DTYPE)
    for g, col in enumerate(np.ascontiguousarray(mv.T).tolist()):
        c = start[:]
        end = n_plies
        ck = cq = ep = 0
        promo = [0] * 5
        for ply, m in enumerate(col):
            if m == NONE:
                end = ply
                break
            f, t, pr = m & 63, (m >> 6) & 63, m >> 12
            pc = c[f]
            kind = pc & 7
            if kind == F.K and abs(t - f) == 2:
                if t > f:
                    ck += 1
                    c[f + 1], c[f + 3] = c[f + 3], -1
                else:
                    cq += 1
                    c[f - 1], c[f - 4] = c[f - 4], -1
            if kind == F.P and (f & 7) != (t & 7) and c[t] < 0:
                ep += 1
                c[(f & ~7) | (t & 7)] = -1
            if pr:
                promo[pr] += 1
                pc = (pc & 8) | pr  # codes 1..4 are the kinds N B R Q
            c[t], c[f] = pc, -1
        assert all(m == NONE for m in col[end:])
        out[g] = (end, ck, cq, ep, promo, O.digest(np.array(c, np.int8), end & 1))
    return out


@functools.lru_cache(maxsize=None)
def big_walk():
    return walk(games(*BIG))


def lone_columns():
    """N_LONE columns of BIG by attribute: four games each that end early, castle,
    promote and capture en passant (the earliest-ending game among them)."""
    w = big_walk()
    n_plies = BIG[3]
    picked = [int(np.argmin(w["end"]))]
    for has in (w["end"] < n_plies, (w["castle_k"] + w["castle_q"]) > 0, w["promo"].sum(axis=1) > 0, w["ep"] > 0):
        fresh = [int(g) for g in np.flatnonzero(has) if g not in picked]
        picked += fresh[:4]
    return picked[:N_LONE]


# ------------------------------------------------------------- 16-bit words
@functools.lru_cache(maxsize=None)
def junk_batch():
    """JUNK_BASE with a seeded JUNK_SHARE of its plies overwritten by (0) a
    random 16-bit word, (1) a legal move with its promotion field changed, (2)
    a legal move with bit 15 set, (3) DC_MOVE_NONE.  An overwritten ply leaves
    the game where it was, so the plies after it no longer fit: a word of the
    base that is no longer legal where it is played is replaced by a seeded
    legal move, and the games keep moving.  Returns (moves, Counter of what
    was written)."""
    base = games(*JUNK_BASE)
    n_plies, n_games = base.shape
    rng = np.random.default_rng(JUNK_BASE[0])
    mv = np.full((n_plies, n_games), NONE, np.uint16)
    what = collections.Counter()
    for g in range(n_games):
        p = O.Pos()
        for ply in range(n_plies):
            legal = O.fast_gen_moves(p, O.FIDE)
            if len(legal) == 0:
                break
            m = int(base[ply, g])
            promos = legal[legal >> 12 != 0]  # rare in 60 plies: where one is legal it is what is spoiled or played
            if rng.random() < JUNK_SHARE:
                kind = 1 if len(promos) else int(rng.integers(0, 4))
                if kind == 0:
                    m = int(rng.integers(0, 1 << 16))
                    what["random"] += 1
                elif kind == 1 and len(promos):
                    pick = int(promos[rng.integers(len(promos))])
                    code = int(rng.choice([0, 5, 6, 7]))
                    m = (pick & 0xFFF) | (code << 12)
                    what["code_removed" if code == 0 else "code_5_to_7"] += 1
                elif kind == 1:
                    code = int(rng.integers(1, 8))
                    m = int(legal[rng.integers(len(legal))]) | (code << 12)
                    what["code_added" if code <= 4 else "code_5_to_7"] += 1
                elif kind == 2:
                    m = int(legal[rng.integers(len(legal))]) | 0x8000
                    what["flagged"] += 1
                else:
                    m = NONE
                    what["none"] += 1
            elif len(promos):
                m = int(promos[rng.integers(len(promos))])
            elif m == NONE or O.fast_validate(p, m, O.FIDE) != O.OK:
                m = int(legal[rng.integers(len(legal))])
                what["repaired"] += 1
            else:
                what["kept"] += 1
            mv[ply, g] = m
            if m != NONE and O.fast_validate(p, m, O.FIDE) == O.OK:
                what["promotion_played"] += bool(m >> 12)
                p = O.fast_make(p, m, O.FIDE)
    mv.flags.writeable = False
    return mv, what


# ------------------------------------------------------------ custom starts
def _special(p, m):
    """Castle, en-passant capture or promotion: the moves that need the start's castle and ep fields."""
    f, t = m & 63, (m >> 6) & 63
    kind = int(p.cells[f]) & 7
    return bool(m >> 12) or (kind == F.K and abs(t - f) == 2) or (kind == F.P and t == p.ep)


@functools.lru_cache(maxsize=None)
def custom_starts():
    """[(label, Pos)]: positions of the constructed set chosen by attribute from
    the set's own model (fide_positions.features), then the six suite FENs."""
    ps = F.position_set()
    feats = [F.features(p, O.fast_gen_moves(p, O.FIDE)) for p in ps]
    chosen = collections.OrderedDict()

    def take(label, pred, k=1):
        hits = [i for i, (p, f) in enumerate(zip(ps, feats)) if i not in chosen and pred(p, f)][:k]
        assert len(hits) == k, label
        for i in hits:
            chosen[i] = label

    for right, stm in ((1, 0), (2, 0), (4, 1), (8, 1)):
        take("only_right_%d" % right, lambda p, f: p.castle == right and p.stm == stm and f["castle_legal"])
    take("ep_white", lambda p, f: p.stm == 0 and f["ep_legal"], 2)
    take("ep_black", lambda p, f: p.stm == 1 and f["ep_legal"], 2)
    take("ep_two", lambda p, f: f["ep_two"])
    take("ep_illegal", lambda p, f: f["ep_illegal"] and not f["ep_legal"], 2)
    take("ep_in_check", lambda p, f: f["ep_in_check"])
    take("double_check", lambda p, f: f["double_check"])
    take("pins2", lambda p, f: f["pins2"], 2)
    take("castle_denied", lambda p, f: f["castle_denied"], 2)
    take("stale_right", lambda p, f: f["stale_right"])
    take("promotion_capture", lambda p, f: f["promotion_capture"])
    take("promotion_white", lambda p, f: p.stm == 0 and f["promotion"])
    take("promotion_black", lambda p, f: p.stm == 1 and f["promotion"])
    take("no_moves", lambda p, f: f["no_moves"])
    take("castle_white", lambda p, f: p.stm == 0 and f["castle_legal"] and p.castle not in (1, 2, 4, 8))
    take("castle_black", lambda p, f: p.stm == 1 and f["castle_legal"] and p.castle not in (1, 2, 4, 8))
    assert len(chosen) >= N_FROM_SET
    out = [("%s_%d" % (label, i), ps[i]) for i, label in chosen.items()]
    out += [("suite_" + name, O.Pos.from_fen(e["fen"])) for name, e in OG["perft_fide"].items()]
    return out


@functools.lru_cache(maxsize=None)
def games_from(index, n_games=64, n_plies=30):
    """Seeded games from custom_starts()[index], built on the host as
    tests/test_gpu_ref.py::_replay_from builds its own: legal moves, 12-bit
    junk, flagged words and early ends (the rest DC_MOVE_NONE).  The first
    plies go through the start's legal moves in turn, castles, en-passant
    captures and promotions first, so each of those is some game's first move;
    promotions with the code taken away or naming no piece come right after."""
    start = custom_starts()[index][1]
    rng = np.random.default_rng(1000 + index)
    legal = [int(m) for m in O.fast_gen_moves(start, O.FIDE)]
    special = [m for m in legal if _special(start, m)]
    # a promotion without its code, and with a code that names no piece
    spoiled = sorted({m & 0xFFF for m in special if m >> 12}) + sorted({(m & 0xFFF) | (6 << 12) for m in special if m >> 12})
    first = special + spoiled[:8] + [m for m in legal if m not in special]
    mv = np.full((n_plies, n_games), NONE, np.uint16)
    for g in range(n_games):
        p = start.copy()
        end = n_plies if rng.random() < 0.8 else int(rng.integers(0, n_plies + 1))
        for ply in range(end):
            r = rng.random()
            legal = O.fast_gen_moves(p, O.FIDE)
            if ply == 0 and g < len(first):
                m = first[g]
            elif r < 0.6 and len(legal):
                m = int(rng.choice(legal))
            elif r < 0.95:
                m = int(rng.integers(0, 4096))
            else:
                m = 0x8000 | int(rng.integers(0, 0x7FFF))
            mv[ply, g] = m
            if O.fast_validate(p, m, O.FIDE) == O.OK:
                p = O.fast_make(p, m, O.FIDE)
    mv.flags.writeable = False
    return mv
